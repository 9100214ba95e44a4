"""Host-only checks of the fused Adam step (no GPU): the entry point's argument checks, the
descriptor layouts shared by include/tlod.h, csrc/optim.hip and tlod/optim.py, and the
optimizer selection of make_optimizer."""
import ctypes
import os
import re

import pytest

from conftest import PKG


def test_adam_argument_checks_host_only():
    """tlod_adam_clip_pack_f32 rejects a null table, n_update > n_chunks, beta = 1 and
    eps = 0 before any device work, and says which."""
    from tlod import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p).value

    def call(chunks=p, n_chunks=2, n_update=2, tiles=None, n_tiles=0, states=p, n_states=1,
             b1=0.9, b2=0.999, eps=1e-8):
        return L.tlod_adam_clip_pack_f32(chunks, n_chunks, n_update, tiles, n_tiles, states,
                                         n_states, 1.0, b1, b2, eps, 10.0, p, p, None)
    assert call(chunks=None) != 0
    assert b"null" in L.tlod_last_error()
    assert call(states=None) != 0
    assert b"null" in L.tlod_last_error()
    assert call(n_update=3) != 0
    assert b"counts" in L.tlod_last_error()
    assert call(n_tiles=1) != 0  # tiles without a tile table
    assert b"counts" in L.tlod_last_error()
    assert call(b1=1.0) != 0
    assert b"beta" in L.tlod_last_error()
    assert call(b2=-0.1) != 0
    assert b"beta" in L.tlod_last_error()
    assert call(eps=0.0) != 0
    assert b"eps" in L.tlod_last_error()
    assert L.tlod_adam_clip_f32(None, 1, p, 1, 1.0, 0.9, 0.999, 1e-8, 10.0, p, p, None) != 0
    assert b"null" in L.tlod_last_error()


def test_descriptor_layouts_match_the_kernels():
    """The numpy dtypes the tables are built with have the sizes csrc/optim.hip asserts of
    the header's structs, and the field order of the header."""
    from tlod import optim
    src = open(os.path.join(PKG, "csrc", "optim.hip")).read()
    sizes = {name: int(n) for name, n in
             re.findall(r"static_assert\(sizeof\((tlod_\w+)\) == (\d+)", src)}
    dtypes = {"tlod_sgd_chunk": optim._DESC, "tlod_sgd_pack_tile": optim._TILE,
              "tlod_adam_chunk": optim._ADAM_DESC, "tlod_adam_pack_tile": optim._ADAM_TILE,
              "tlod_adam_state": optim._ADAM_STATE}
    assert sorted(sizes) == sorted(dtypes)
    for name, dt in dtypes.items():
        assert dt.itemsize == sizes[name], name
    header = open(os.path.join(os.path.dirname(PKG), "include", "tlod.h")).read()
    alias = {"momentum_buf": "buf", "weight_decay": "wd"}
    for name in ("tlod_adam_chunk", "tlod_adam_pack_tile", "tlod_adam_state"):
        body = re.search(r"typedef struct %s \{(.*?)\}" % name, header, re.S).group(1)
        fields = []
        for decl in body.split(";"):
            fields += re.findall(r"(\w+)\s*(?:,|$)", decl.strip().replace("*", " "))
        fields = [alias.get(f, f) for f in fields]
        assert fields == list(dtypes[name].names), name


def test_make_optimizer_rejects_unknown_name():
    import torch
    from tlod.detector.train import make_optimizer
    with pytest.raises(ValueError, match="lion"):
        make_optimizer(torch.nn.Linear(2, 2), 1e-3, optimizer="lion")


@pytest.mark.parametrize("flag", ["amsgrad", "maximize", "decoupled_weight_decay"])
def test_adam_rejects_unsupported_variants(flag):
    import torch
    from tlod.optim import FusedAdamClip
    w = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError, match=flag):
        FusedAdamClip([{"params": [w], "lr": 1e-3, "weight_decay": 0.0, flag: True}])
    with pytest.raises(ValueError, match="betas"):
        FusedAdamClip([{"params": [w], "lr": 1e-3}], betas=(0.9, 1.0))
