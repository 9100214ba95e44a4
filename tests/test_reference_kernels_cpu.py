"""The reference-kernel recipe (oracle/ref_build.py), build()'s hook and the host-side
validators of oracle/ref_kernels.py, without a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import ref_build
from oracle import ref_kernels as rk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_build_reference_into_temp_dir(tmp_path):
    """With a checkout: both libraries appear, all seven entry points bind through ctypes, and a
    second call rebuilds nothing."""
    ref_dir = ref_build.find_reference()
    if ref_dir is None:
        pytest.skip("no reference checkout ($TLOD_REFERENCE_DIR or ../reference)")
    out = str(tmp_path / "_ref")
    built = ref_build.build_reference(ref_dir, out)
    assert sorted(os.path.basename(b) for b in built) == ["libtlod_ref.so", "libtlod_ref_fma.so"]
    for b in built:
        L = rk.bind(b)
        for name in ref_build.SYMBOLS:
            assert isinstance(getattr(L, name), ctypes._CFuncPtr), name
    assert set(ref_build.SYMBOLS) == set(rk.SIGNATURES)
    stamps = {b: os.stat(b).st_mtime_ns for b in built}
    assert ref_build.build_reference(ref_dir, out) == []
    assert {b: os.stat(b).st_mtime_ns for b in built} == stamps


def test_recipe_commands(tmp_path, monkeypatch):
    """The commands the recipe issues, on a stand-in checkout of empty files: the four sources
    compiled in place (no copy), -O2, gfx950, the shim force-included, -ffp-contract=off in the
    first build only, no fast-math or division flags, at most 16 at a time."""
    ref = tmp_path / "ref"
    for s in ref_build.SOURCES:
        (ref / s).parent.mkdir(parents=True, exist_ok=True)
        (ref / s).write_text("")
    cmds = []
    monkeypatch.setattr(ref_build.subprocess, "run", lambda cmd, check: cmds.append(cmd))
    out = tmp_path / "out"
    ref_build.build_reference(str(ref), str(out))
    compiles = [c for c in cmds if "-c" in c]
    links = [c for c in cmds if "-shared" in c]
    assert len(compiles) == 8 and len(links) == 2 and ref_build.MAX_JOBS <= 16
    for c in compiles:
        assert "--offload-arch=gfx950" in c and "-O2" in c and "-fPIC" in c
        assert c[c.index("-include") + 1] == ref_build.SHIM
        assert c[c.index("-c") + 1].startswith(str(ref))  # straight from the checkout
        assert not any(a.startswith("-") and ("fast-math" in a or "div" in a or a == "-Ofast")
                       for a in c)
    off = [c for c in compiles if "obj_libtlod_ref" + os.sep in c[-1]]
    fma = [c for c in compiles if "obj_libtlod_ref_fma" + os.sep in c[-1]]
    assert len(off) == 4 and all("-ffp-contract=off" in c for c in off)
    assert len(fma) == 4 and not any(a.startswith("-ffp-contract") for c in fma for a in c)
    assert sorted(os.path.basename(c[c.index("-o") + 1]) for c in links) == sorted(ref_build.VARIANTS)
    assert not [p for p in out.rglob("*") if p.suffix in (".cu", ".h")]


def test_build_hook_without_checkout_is_a_noop(tmp_path, monkeypatch, capsys):
    import __graft_entry__ as entry
    monkeypatch.setenv(ref_build.ENV, str(tmp_path / "nowhere"))
    monkeypatch.setattr(ref_build, "ROOT", str(tmp_path / "repo"))  # nothing beside it either
    called = []
    monkeypatch.setattr(ref_build, "build_reference", lambda *a, **k: called.append(a))
    assert ref_build.find_reference() is None
    entry._build_reference_kernels()
    assert called == []
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1 and "no reference checkout" in lines[0]


def test_failed_compile_fails_the_build_and_leaves_no_stale_library(tmp_path, monkeypatch):
    """With a checkout present, a compile failure propagates out of build()'s hook, and the
    libraries of an earlier build are gone (the GPU module cannot run against stale ones)."""
    import __graft_entry__ as entry
    ref = tmp_path / "ref"
    for s in ref_build.SOURCES:
        (ref / s).parent.mkdir(parents=True, exist_ok=True)
        (ref / s).write_text("")
    out = tmp_path / "out"
    out.mkdir()
    for name in ref_build.VARIANTS:
        (out / name).write_text("old")
    os.utime(ref / ref_build.SOURCES[0])  # a source newer than the old libraries

    def boom(cmd, check):
        raise subprocess.CalledProcessError(1, cmd)
    monkeypatch.setattr(ref_build.subprocess, "run", boom)
    monkeypatch.setenv(ref_build.ENV, str(ref))
    monkeypatch.setattr(ref_build, "DEFAULT_OUT", str(out))
    with pytest.raises(subprocess.CalledProcessError):
        entry._build_reference_kernels()
    assert not [p for p in out.iterdir() if p.suffix == ".so"]


# ------------------------------------------------------------------ validators
@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load (or call into) the library fails the test."""
    def refuse(*a, **k):
        raise AssertionError("the library was touched before validation finished")
    monkeypatch.setattr(rk.ctypes, "CDLL", refuse)
    monkeypatch.setattr(rk, "_load", refuse)
    monkeypatch.setattr(rk, "_loaded", {})


def _feat(B=2, C=3, H=6, W=7):
    return torch.arange(B * C * H * W, dtype=torch.float32).reshape(B, C, H, W)


def _rois(B=2):
    r = torch.tensor([[0, 4, 4, 40, 40], [1, 8, 8, 60, 50], [0, 0, 0, 10, 10],
                      [1, 20, 10, 90, 70]], dtype=torch.float32)
    r[:, 0] = r[:, 0].clamp(max=B - 1)
    return r


def _grid(R=4, G=3):
    return torch.zeros((R, G, G, 2), dtype=torch.float32)


def _calls(feat, rois, ah=4, aw=4, P=3):
    """Every RoI entry point of the wrapper on (feat, rois)."""
    B, C, H, W = feat.shape
    R = rois.shape[0]
    return {
        "align_fwd": lambda: rk.roi_align_fwd(feat, rois, ah, aw, 1 / 16),
        "align_bwd": lambda: rk.roi_align_bwd(torch.zeros(R, C, ah, aw), rois, B, C, H, W, 1 / 16),
        "pool_fwd": lambda: rk.roi_pool_fwd(feat, rois, P, P, 1 / 16),
        "pool_bwd": lambda: rk.roi_pool_bwd(torch.zeros(R, C, P, P),
                                            torch.zeros(R, C, P, P, dtype=torch.int32), rois,
                                            B, C, H, W, 1 / 16),
    }


def test_valid_cpu_inputs_reach_only_the_device_check(no_library):
    for name, call in _calls(_feat(), _rois()).items():
        with pytest.raises(ValueError, match="CUDA"):
            call()
    with pytest.raises(ValueError, match="CUDA"):
        rk.roi_crop_fwd(_feat(), _grid())
    with pytest.raises(ValueError, match="CUDA"):
        rk.roi_crop_bwd(_feat(), _grid(), torch.zeros(4, 3, 3, 3))
    with pytest.raises(ValueError, match="CUDA"):
        rk.nms(torch.tensor([[0, 0, 10, 10, 1.0]]), 0.7)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_rejects_nonfinite_roi(no_library, bad):
    r = _rois()
    r[2, 3] = bad
    for name, call in _calls(_feat(), r).items():
        with pytest.raises(ValueError, match="finite"):
            call()
    g = _grid()
    g[1, 0, 0, 1] = bad
    with pytest.raises(ValueError, match="finite"):
        rk.roi_crop_fwd(_feat(), g)
    d = torch.tensor([[0, 0, 10, 10, 1.0], [0, bad, 5, 5, 0.5]])
    with pytest.raises(ValueError, match="finite"):
        rk.nms(d, 0.7)


@pytest.mark.parametrize("idx", [2.0, -1.0, 0.5])
def test_rejects_batch_index_outside_the_batch(no_library, idx):
    r = _rois()
    r[1, 0] = idx  # B = 2: index B itself, a negative one, a fractional one
    for name, call in _calls(_feat(), r).items():
        with pytest.raises(ValueError, match="batch indices"):
            call()


def test_rejects_one_row_or_one_column_maps(no_library):
    for feat in (_feat(H=1), _feat(W=1)):
        for name, call in _calls(feat, _rois()).items():
            with pytest.raises(ValueError, match="H, W >= 2"):
                call()
        with pytest.raises(ValueError, match="H, W >= 2"):
            rk.roi_crop_fwd(feat, _grid())


def test_rejects_aligned_size_one(no_library):
    for ah, aw in ((1, 4), (4, 1)):
        calls = _calls(_feat(), _rois(), ah=ah, aw=aw)
        for name in ("align_fwd", "align_bwd"):
            with pytest.raises(ValueError, match="aligned"):
                calls[name]()


def test_rejects_noncontiguous_and_wrong_dtype(no_library):
    feat = _feat(H=7, W=6).transpose(2, 3)
    assert not feat.is_contiguous()
    for name in ("align_fwd", "pool_fwd"):
        with pytest.raises(ValueError, match="contiguous"):
            _calls(feat, _rois())[name]()
    with pytest.raises(ValueError, match="contiguous"):
        rk.roi_align_fwd(_feat(), torch.zeros(5, 4).t(), 4, 4, 1 / 16)
    with pytest.raises(ValueError, match="contiguous"):
        rk.roi_crop_fwd(_feat(), torch.zeros(4, 3, 2, 3).transpose(2, 3))
    with pytest.raises(ValueError, match="contiguous"):
        rk.nms(torch.zeros(5, 4).t(), 0.7)
    with pytest.raises(ValueError, match="float32"):
        rk.roi_align_fwd(_feat().double(), _rois(), 4, 4, 1 / 16)


def test_rejects_crop_roi_count_no_multiple_of_batch(no_library):
    with pytest.raises(ValueError, match="multiple"):
        rk.roi_crop_fwd(_feat(), _grid(R=3))
    with pytest.raises(ValueError, match="multiple"):
        rk.roi_crop_bwd(_feat(), _grid(R=3), torch.zeros(3, 3, 3, 3))


def test_rejects_far_grid_and_far_roi(no_library):
    g = _grid()
    g[0, 0, 0, 0] = 8.5
    with pytest.raises(ValueError, match="<= 8"):
        rk.roi_crop_fwd(_feat(), g)
    r = _rois()
    r[0, 3] = 1e9
    for name, call in _calls(_feat(), r).items():
        with pytest.raises(ValueError, match="2\\^20"):
            call()


def test_rejects_element_counts_of_2_31(no_library):
    # a (1, 1, 2, 2) map expanded without memory would not be contiguous: use the count check
    with pytest.raises(ValueError, match="2\\^31"):
        rk._check_count("x", 2 ** 31)
    rk._check_count("x", 2 ** 31 - 1)
    with pytest.raises(ValueError, match="2\\^31"):  # R * C * ah * aw
        rk._check_align(_feat(B=1, C=1), _rois(B=1), 2 ** 16, 2 ** 15, 1 / 16)


# ------------------------------------------------------------------ nothing built is tracked
def test_reference_binaries_are_not_tracked():
    ignore = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "oracle/_ref/" in ignore
    p = subprocess.run(["git", "-C", ROOT, "ls-files", "oracle/_ref"], capture_output=True,
                       text=True)
    if p.returncode == 0:  # (an exported tree has no git metadata: the ignore rule is the check)
        assert p.stdout.strip() == ""
