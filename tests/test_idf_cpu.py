"""IDF without a GPU: the restated ops (tests/ref_idf.py) against autograd in fp64, the a == b
corner of the distance, the torch compositions of tlod.da.idf against the restatement, the
method's plumbing (METHODS, state_dict names, frozen dead modules, no clipping), the target
call's zero-box proposal target, and the extension-ABI ledger: include/tlod_idf.h ==
tlod._lib.EXT_SIGNATURES, the library exports every name, and every name has a guard-band case
in tests/test_idf_abi_gpu.py or is a host-only *_workspace_bytes query."""
import ast
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(ROOT, "include", "tlod_idf.h")


# ---------------------------------------------------------------- the restated ops
def test_distance_and_modulation_gradcheck():
    from ref_idf import distance, modulate
    torch.manual_seed(0)
    a = torch.randn(1, 8, 3, 5, dtype=torch.float64, requires_grad=True)
    b = torch.randn(1, 8, 3, 5, dtype=torch.float64, requires_grad=True)
    att_a = torch.rand(1, 1, 3, 5, dtype=torch.float64)
    att_b = torch.rand(1, 1, 3, 5, dtype=torch.float64)
    att_b[0, 0, 1, 2] = 0.0
    assert torch.autograd.gradcheck(lambda x, y: distance(x, y, att_b), (a, b))
    assert torch.autograd.gradcheck(lambda x, y: distance(x, y), (a, b))
    assert torch.autograd.gradcheck(lambda x, y: modulate(x, y, att_a, att_b), (a, b))


def test_separation_backward_formula_is_the_autograd_gradient():
    """The kernel's statement — t = g / (H W) att_b ((a - b) att_b + 1e-6) / d, g_a = g_a_out
    (1 + att_b) + t, g_b = g_b_out (1 + att_a) - t — against autograd in fp64."""
    from ref_idf import distance, modulate
    torch.manual_seed(1)
    a = torch.randn(2, 8, 3, 5, dtype=torch.float64, requires_grad=True)
    b = torch.randn(2, 8, 3, 5, dtype=torch.float64, requires_grad=True)
    att_a = torch.rand(2, 1, 3, 5, dtype=torch.float64)
    att_b = torch.rand(2, 1, 3, 5, dtype=torch.float64)
    ga_out, gb_out = torch.randn_like(a), torch.randn_like(b)
    g_dist = torch.tensor([0.7, -1.3], dtype=torch.float64)
    ao, bo = modulate(a, b, att_a, att_b)
    ((ao * ga_out).sum() + (bo * gb_out).sum() + (distance(a, b, att_b) * g_dist).sum()).backward()
    with torch.no_grad():
        e = (a - b) * att_b + 1e-6
        d = e.norm(2, dim=1, keepdim=True)
        t = g_dist.view(2, 1, 1, 1) / 15 * att_b * e / d
        assert torch.allclose(a.grad, ga_out * (1 + att_b) + t, rtol=1e-12, atol=1e-14)
        assert torch.allclose(b.grad, gb_out * (1 + att_a) - t, rtol=1e-12, atol=1e-14)


def test_dam_by_hand_and_per_image_thresholds():
    from ref_idf import dam
    x = torch.zeros(2, 4, 1, 3)
    x[0, :, 0, 0], x[0, :, 0, 2] = 4.0, -4.0      # avg: s(4), 0.5, s(-4); thr = 0.5
    x[1] = 10.0
    x[1, :, 0, 1] = 9.0                            # image 1 lives far above image 0's threshold
    att = dam(x)
    s = lambda v: 1 / (1 + math.exp(-v))
    assert att.shape == (2, 1, 1, 3)
    np.testing.assert_allclose(att[0, 0, 0].numpy(), [s(4.0), 0.5, 0.0], rtol=1e-6)
    # its own threshold zeroes image 1's lowest cell; a batch-wide mean would keep all three
    assert att[1, 0, 0, 1] == 0 and att[1, 0, 0, 0] > 0.99 and att[1, 0, 0, 2] > 0.99
    for n in range(2):
        assert torch.equal(dam(x[n:n + 1]), att[n:n + 1])


def test_equal_maps_give_sqrt_c_eps_and_finite_gradients():
    from ref_idf import distance
    a = torch.randn(1, 24, 5, 7, dtype=torch.float64, requires_grad=True)
    b = a.detach().clone().requires_grad_(True)
    att = torch.rand(1, 1, 5, 7, dtype=torch.float64)
    dist = distance(a, b, att)
    assert abs(dist.item() - math.sqrt(24) * 1e-6) < 1e-12   # 4.899e-6
    dist.sum().backward()
    assert torch.isfinite(a.grad).all() and torch.isfinite(b.grad).all()
    assert torch.equal(a.grad, -b.grad)


def test_focal_loss_gradcheck_clamp_and_by_hand():
    from ref_idf import focal_loss
    torch.manual_seed(2)
    z = torch.randn(6, 2, dtype=torch.float64, requires_grad=True)
    for label in (0, 1):
        assert torch.autograd.gradcheck(lambda x: focal_loss(x, label, 3.0), (z,))
    z = torch.tensor([[0.0, 0.0], [20.0, 0.0]], dtype=torch.float64, requires_grad=True)
    loss = focal_loss(z, 1, 3.0)
    # row 0: p = 0.5; row 1: softmax[1] = 2e-9 < 1e-6 -> clamped, no gradient
    want = (0.5 ** 3 * math.log(2.0) + (1 - 1e-6) ** 3 * -math.log(1e-6)) / 2
    assert abs(loss.item() - want) < 1e-12
    loss.backward()
    assert z.grad[1].abs().max() == 0 and z.grad[0].abs().min() > 0


def test_module_compositions_equal_the_restatement():
    """TLOD_FUSED_IDF=0's torch forms (tlod.da.idf) against tests/ref_idf.py."""
    import ref_idf
    from tlod.da import idf
    torch.manual_seed(3)
    a, b = torch.randn(2, 24, 5, 7), torch.randn(2, 24, 5, 7)
    att_a, att_b = idf.dam_torch(a), idf.dam_torch(b)
    assert torch.equal(att_a, ref_idf.dam(a)[:, 0])
    ao, bo, d, dist = idf.separation_torch(a, b, att_a, att_b)
    ra, rb = ref_idf.modulate(a, b, att_a.unsqueeze(1), att_b.unsqueeze(1))
    assert torch.equal(ao, ra) and torch.equal(bo, rb)
    assert torch.allclose(dist, ref_idf.distance(a, b, att_b.unsqueeze(1)), rtol=1e-6)
    assert torch.allclose(idf.separation_torch(a, b, None, None, False)[3],
                          ref_idf.distance(a, b), rtol=1e-6)
    z_img, z_ins = torch.randn(6, 2), torch.randn(9, 2) * 8
    for label in (0, 1):
        got = idf.domain_losses_torch(z_img, label, z_ins, label, 3.0)
        want = [ref_idf.cross_entropy2(z_img[i:i + 1], label) for i in range(6)]
        want.append(ref_idf.focal_loss(z_ins, label, 3.0))
        assert torch.allclose(got, torch.stack(want), rtol=1e-6, atol=1e-7)


# ---------------------------------------------------------------- plumbing
def test_method_is_listed_and_has_no_resnet():
    from tlod.detector.train import METHODS, build_model
    assert "idf" in METHODS
    with pytest.raises(NotImplementedError):
        build_model("idf", "cpu", "res101")


def test_state_dict_names_frozen_parts_and_oracle_load():
    from ref_idf import OracleIDF
    from tlod.detector.train import build_model, make_optimizer
    m = build_model("idf", "cpu")
    sd = m.state_dict()
    want = {"RCNN_base1.0.weight": (64, 3, 3, 3), "RCNN_base1_b.0.weight": (64, 3, 3, 3),
            "RCNN_base1.12.weight": (256, 256, 3, 3), "RCNN_base2.0.weight": (256, 256, 3, 3),
            "RCNN_base2.5.weight": (512, 512, 3, 3), "RCNN_base3_b.7.weight": (512, 512, 3, 3),
            "netD_1.conv1.weight": (256, 256, 1, 1), "netD_1_b.conv3.weight": (128, 128, 1, 1),
            "netD_2.conv1.weight": (512, 512, 3, 3), "netD_3_b.conv2.weight": (128, 512, 3, 3),
            "netD_2.bn1.running_mean": (512,), "netD_3.fc.weight": (2, 128),
            "netD_da.fc1.weight": (100, 4096), "netD_da.bn2.weight": (100,),
            "netD_da.fc3.bias": (2,), "fuse_3.conv3.weight": (512, 512, 3, 3),
            "fuse_3.conv1.weight": (512, 512, 1, 1), "RCNN_rpn_t.RPN_Conv.weight": (512, 512, 3, 3),
            "RCNN_top_t.3.weight": (4096, 4096), "RCNN_cls_score_t.weight": (9, 4096),
            "RCNN_bbox_pred_t.bias": (36,)}
    for k, shape in want.items():
        assert k in sd and tuple(sd[k].shape) == shape, (k, sd.get(k, torch.empty(0)).shape)
    # the frozen conv1 / conv2 prefix is one set of tensors under both stacks' keys
    for i in (0, 2, 5, 7):
        assert sd[f"RCNN_base1.{i}.weight"].data_ptr() == sd[f"RCNN_base1_b.{i}.weight"].data_ptr()
    assert sd["RCNN_base1.10.weight"].data_ptr() != sd["RCNN_base1_b.10.weight"].data_ptr()
    named = dict(m.named_parameters())
    dead = [p for k, p in named.items() if k.startswith("fuse_3.")]
    assert len(dead) == 4 and not any(p.requires_grad for p in dead)
    assert not named["RCNN_base1.7.weight"].requires_grad and named["RCNN_base1.10.weight"].requires_grad
    ids = {id(p) for g in make_optimizer(m, 1e-3, fused=False).param_groups for p in g["params"]}
    assert not any(id(p) in ids for p in dead)
    assert id(m.netD_da.fc3.weight) in ids and id(m.RCNN_bbox_pred_t.weight) in ids
    o = OracleIDF(dropout=0.0)
    o.load_state_dict(sd, strict=True)
    assert {k for k, p in o.named_parameters() if p.requires_grad} == \
        {k for k, p in named.items() if p.requires_grad}
    assert m.netD_2.drop_p == 0.5 and m.netD_da.drop_p == 0.5


def test_clipping_idf_none_daf_unchanged():
    from tlod.detector.train import build_model, default_clip
    assert default_clip(build_model("idf", "cpu")) == 0.0
    daf = build_model("daf", "cpu")
    assert not hasattr(daf, "clip_norm") and default_clip(daf) == 10.0
    daf.net = "res101"
    assert default_clip(daf) == 0.0


def test_forward_needs_the_pseudo_boxes_in_training():
    from tlod.detector.train import build_model
    m = build_model("idf", "cpu")
    with pytest.raises(RuntimeError, match="6-argument"):
        m(*[torch.zeros(1)] * 4)


def test_synthetic_batches_default_unchanged_and_pseudo_boxes():
    from tlod.detector.train import SyntheticCityscapes
    a = SyntheticCityscapes("cpu", H=64, W=96, G=3, pool=2, seed=5)
    b = SyntheticCityscapes("cpu", H=64, W=96, G=3, pool=2, seed=5, tgt_G=0)
    for x, y in zip(a.batches, b.batches):
        assert all(torch.equal(s, t) for s, t in zip(x, y))
    c = SyntheticCityscapes("cpu", H=64, W=96, G=3, pool=1, seed=5, tgt_G=2).batches[0]
    d = a.batches[0]
    assert all(torch.equal(c[i], d[i]) for i in (0, 1, 2, 3, 4, 5, 6, 9))
    assert tuple(d[7].shape) == (1, 5) and int(d[8]) == 0
    assert tuple(c[7].shape) == (1, 50, 5) and int(c[8]) == 2
    assert (c[7][0, :2, 4] >= 1).all() and (c[7][0, 2:] == 0).all()
    assert (c[7][0, :2, 2] > c[7][0, :2, 0]).all()


def test_zero_box_proposal_target_samples_256_background_rois():
    """The target call's main-stack proposal target: one all-zero gt box, BG_THRESH_LO = 0.
    Every proposal has overlap 0 with it (background); the appended zero box itself has
    overlap -1 and is never drawn."""
    from helpers import random_boxes
    from oracle import rpn as orpn
    assert orpn.DEFAULT_RCNN["bg_lo"] == 0.0
    rng = np.random.default_rng(0)
    R = 300
    rois = np.zeros((1, R, 5), np.float32)
    rois[0, :, 1:] = random_boxes(rng, R, W=320, H=192)
    rois[0, -20:] = 0  # the proposal layer's zero padding
    out, labels, targets, inside, outside = orpn.proposal_target(
        rois, np.zeros((1, 1, 5), np.float32), np.random.RandomState(3))
    assert out.shape == (1, 256, 5) and (labels == 0).all()
    assert (targets == 0).all() and (inside == 0).all() and (outside == 0).all()
    picked = {tuple(r) for r in out[0, :, 1:].tolist()}
    assert picked <= {tuple(r) for r in rois[0, :-20, 1:].tolist()} and len(picked) > 100


# ---------------------------------------------------------------- the extension ledger
def declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tlod_[a-z0-9_]+)\s*\(", src)))


def guarded_calls():
    """Entry points handed to Call.run as L.<name> in tests/test_idf_abi_gpu.py (the rule of
    tests/test_abi_guard_cpu.py: a name in a comment or a string does not count)."""
    tree = ast.parse(open(os.path.join(HERE, "test_idf_abi_gpu.py")).read())
    called = set()
    for n in ast.walk(tree):
        if (isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "run"
                and n.args):
            f = n.args[0]
            if (isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name)
                    and f.value.id == "L" and f.attr.startswith("tlod_")):
                called.add(f.attr)
    return called


def test_extension_header_matches_the_table_and_the_library():
    from tlod import _lib
    syms = declared()
    assert syms and sorted(_lib.EXT_SIGNATURES) == syms
    assert not set(syms) & set(_lib.SIGNATURES)
    assert os.path.exists(_lib.LIB_PATH), "build libtlod.so first (__graft_entry__.build())"
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert not [s for s in syms if not hasattr(L, s)]
    bound = _lib.lib()
    for name, (res, args) in _lib.EXT_SIGNATURES.items():
        fn = getattr(bound, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_extension_ledger_covers_every_entry_point():
    from tlod import _lib
    host_only = {n for n in _lib.EXT_SIGNATURES if n.endswith("_workspace_bytes")}
    assert host_only == {"tlod_idf_dam_workspace_bytes", "tlod_idf_sep_fwd_workspace_bytes"}
    assert guarded_calls() == set(_lib.EXT_SIGNATURES) - host_only


def test_host_only_queries_and_argument_checks():
    from tlod import _lib
    L = _lib.lib()
    assert L.tlod_idf_dam_workspace_bytes(1, 75, 150) == 176 * 8 + (-176 * 8) % 256
    assert L.tlod_idf_sep_fwd_workspace_bytes(2, 37, 75) == 2 * 44 * 8 + (-2 * 44 * 8) % 256
    assert L.tlod_idf_dam_workspace_bytes(0, 5, 5) == 0
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    assert L.tlod_idf_dam_f32(p, 1, 0, 5, 7, p + 16, p, 256, None) == -1
    assert L.tlod_idf_dam_f32(p, 1, 4, 5, 7, p + 16, None, 0, None) == -3
    assert b"workspace" in L.tlod_last_error()
    assert L.tlod_idf_sep_fwd_f32(p, p, None, None, 1, 4, 5, 7, p + 8, None, p, p, p, 256, None) == -1
    assert b"both or neither" in L.tlod_last_error()
    assert L.tlod_idf_sep_fwd_f32(p, p, None, None, 1, 4, 5, 7, p + 8, p + 16, p, p, p, 256,
                                  None) == -1
    assert b"att_a and att_b" in L.tlod_last_error()
    assert L.tlod_idf_sep_bwd_f32(p, p, None, None, p, p, None, p, 1, 4, 5, 7, p, p, None) == -1
    assert L.tlod_idf_domain_loss_f32(p, 6, 2, p, 4, 0, 3.0, p, None) == -1
    assert b"labels" in L.tlod_last_error()
    assert L.tlod_idf_domain_loss_bwd_f32(p, 6, 0, p, 0, 0, 3.0, p, p, p, None) == -1
