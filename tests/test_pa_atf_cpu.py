"""PA-ATF's device ops without a GPU: the extension-ABI ledger (include/tlod_pa_atf.h ==
tlod._lib.PA_ATF_SIGNATURES, disjoint from the other two tables, every name exported and bound,
every entry with a guard-band case in tests/test_pa_atf_abi_gpu.py), the host-only argument
checks, StridedConv2d as an nn.Conv2d (parameters, init, state_dict keys, the TLOD_SCONV=0
path), and the torch compositions of tlod.da.pa_atf against the reference's formulas."""
import ast
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(ROOT, "include", "tlod_pa_atf.h")


# ---------------------------------------------------------------- the extension ledger
def declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(tlod_[a-z0-9_]+)\s*\(", src)))


def guarded_calls():
    """Entry points handed to Call.run as L.<name> in tests/test_pa_atf_abi_gpu.py (the rule of
    tests/test_idf_cpu.py: a name in a comment or a string does not count)."""
    tree = ast.parse(open(os.path.join(HERE, "test_pa_atf_abi_gpu.py")).read())
    called = set()
    for n in ast.walk(tree):
        if (isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "run"
                and n.args):
            f = n.args[0]
            if (isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name)
                    and f.value.id == "L" and f.attr.startswith("tlod_")):
                called.add(f.attr)
    return called


def test_header_matches_the_table_and_the_library():
    from tlod import _lib
    syms = declared()
    assert syms and sorted(_lib.PA_ATF_SIGNATURES) == syms
    assert not set(syms) & set(_lib.SIGNATURES)
    assert not set(syms) & set(_lib.EXT_SIGNATURES)
    assert os.path.exists(_lib.LIB_PATH), "build libtlod.so first (__graft_entry__.build())"
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert not [s for s in syms if not hasattr(L, s)]
    bound = _lib.lib()
    for name, (res, args) in _lib.PA_ATF_SIGNATURES.items():
        fn = getattr(bound, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_ledger_covers_every_entry_point():
    from tlod import _lib
    host_only = {n for n in _lib.PA_ATF_SIGNATURES if n.endswith("_workspace_bytes")}
    assert host_only == {"tlod_proposal_subsample_workspace_bytes"}
    assert guarded_calls() == set(_lib.PA_ATF_SIGNATURES) - host_only


def test_argument_checks_refuse_before_any_launch():
    from tlod import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    for fn in (L.tlod_im2col_f32, L.tlod_col2im_f32):
        assert fn(p, 1, 2, 8, 8, 0, 1, 0, p, None) == -1        # KS < 1
        assert b"KS >= 1" in L.tlod_last_error()
        assert fn(p, 1, 2, 8, 8, 3, 0, 0, p, None) == -1        # stride < 1
        assert fn(p, 1, 2, 8, 8, 3, 2, -1, p, None) == -1       # pad < 0
        assert fn(p, 1, 2, 4, 8, 5, 3, 0, p, None) == -1        # H < KS: no 1 x 1 output
        assert fn(p, 1, 2, 8, 2, 5, 3, 1, p, None) == -1        # W + 2 pad < KS
        assert fn(None, 1, 2, 8, 8, 3, 2, 0, p, None) == -1
        assert b"null pointer" in L.tlod_last_error()
        assert fn(p, 0, 2, 8, 8, 3, 2, 0, p, None) == -1
    assert L.tlod_pa_gate_f32(p, 1, 0, 3, 3, p, p, None) == -1
    assert L.tlod_pa_gate_f32(p, 1, 4, 3, 3, p, None, None) == -1
    assert L.tlod_pa_gate_bwd_f32(p, p, p, 1, 4, 0, 3, p, None) == -1
    assert L.tlod_pa_proto_pool_fwd_f32(p, 4, 5, 5, p, 0, 0.25, p, p, p, p, p, None) == -1
    assert b"bad shape" in L.tlod_last_error()
    assert L.tlod_pa_proto_pool_fwd_f32(p, 4, 5, 5, p, 1, 0.25, p, None, p, p, p, None) == -1
    assert L.tlod_pa_proto_pool_bwd_f32(p, p, p, p, p, p, 1, 0.25, 4, 0, 5, 0.1, p, None) == -1
    # the subsampled proposal layer: head > post, and a workspace one byte short
    assert L.tlod_proposal_pick_f32(p, p, 1, 64, 16, 17, None, None, 0, p, None) == -1
    assert b"head <= post" in L.tlod_last_error()
    assert L.tlod_proposal_pick_f32(p, p, 1, 64, 16, 4, p, None, 0, p, None) == -1
    assert b"both or neither" in L.tlod_last_error()
    assert L.tlod_proposal_pick_f32(p, p, 1, 16385, 16, 4, None, None, 0, p, None) == -4
    q = L.tlod_proposal_workspace_bytes(1, 12, 5, 7, 300)
    assert L.tlod_proposal_keep_f32(p, p, p, p, 1, 12, 5, 7, 16, 300, 0.7, p, p, p, q - 1,
                                    None) == -3
    assert b"workspace" in L.tlod_last_error()
    qs = L.tlod_proposal_subsample_workspace_bytes(1, 12, 5, 7, 300)
    assert qs >= q + 300 * 16 + 4 and qs % 256 == 0
    assert L.tlod_proposal_subsample_f32(p, p, p, p, 1, 12, 5, 7, 16, 300, 64, 16, 0.7, 0, p, p,
                                         qs - 1, None) == -3
    assert L.tlod_proposal_subsample_f32(p, p, p, p, 1, 12, 5, 7, 16, 300, 64, 65, 0.7, 0, p, p,
                                         qs, None) == -1


def test_subsample_rule_on_hand_made_keep_lists():
    """lib/PA_ATF/proposal_layer1.py:152-160 of the reference, literally, against
    tlod.rpn.proposal.subsample_rule: keep lists shorter than head, between head and post, and
    longer than post."""
    import numpy as np
    from tlod.rpn.proposal import subsample_head, subsample_rule
    post = 256
    assert subsample_head(post) == int(post * 0.25) == 64
    for n in (0, 10, 64, 65, 200, 256, 257, 1750):
        keep = [1000 + 3 * i for i in range(n)]
        perm = np.random.RandomState(n).permutation(max(n - 64, 0))
        rows, idx = subsample_rule(keep, post, lambda m: perm)
        other = keep[int(post * 0.25):]                         # the reference's lines
        first = keep[:int(post * 0.25)]
        k = min(len(other), int(post * 0.75))
        want = first + [other[i] for i in perm[:k]]
        assert rows == want and len(rows) == min(n, 64) + min(max(n - 64, 0), 192)
        assert len(set(rows)) == len(rows) <= post and idx == [int(i) for i in perm[:k]]
        assert rows[:64] == keep[:64]


# ---------------------------------------------------------------- plumbing
def test_method_is_listed_and_has_no_resnet():
    from tlod.detector.train import METHODS, build_model
    assert "pa_atf" in METHODS
    with pytest.raises(NotImplementedError):
        build_model("pa_atf", "cpu", "res101")


def test_state_dict_names_shapes_and_restatement_load():
    from ref_pa_atf import OraclePAATF
    from tlod.conv import Conv2d, StridedConv2d
    from tlod.detector.train import build_model, default_clip
    m = build_model("pa_atf", "cpu")
    sd = m.state_dict()
    want = {"RCNN_base.10.weight": (256, 128, 3, 3), "RCNN_base_t.10.weight": (256, 128, 3, 3),
            "conv3_s.0.weight": (64, 3, 3, 3), "conv3_t.14.weight": (256, 256, 3, 3),
            "conv34_s.1.weight": (512, 256, 3, 3), "conv34_t.5.bias": (512,),
            "conv45_s.1.weight": (512, 512, 3, 3), "conv45_t.5.weight": (512, 512, 3, 3),
            "RCNN_imageDA_3.Conv1.weight": (128, 256, 1, 1),
            "RCNN_imageDA_3.Conv2.weight": (1, 128, 1, 1),
            "RCNN_imageDA_3.Convm1.weight": (256, 256, 5, 5), "RCNN_imageDA_3.Convm1.bias": (256,),
            "RCNN_imageDA_4.Convm2.weight": (512, 512, 3, 3), "RCNN_imageDA_4.Convm2.bias": (512,),
            "RCNN_imageDA.Conv1.weight": (256, 512, 1, 1), "RCNN_imageDA.Convm1.weight": (512, 512, 5, 5),
            "RCNN_instanceDA.dc_ip1.weight": (1024, 4096), "RCNN_instanceDA.dc_ip2.bias": (1024,),
            "RCNN_instanceDA.clssifer.weight": (1, 1024),
            "club3.out_score.0.weight": (256, 512, 3, 3), "club3.out_score.2.weight": (128, 256, 1, 1),
            "club4.out_score.0.weight": (512, 1024, 3, 3), "club5.out_score.2.bias": (128,),
            "club5.fc.weight": (2, 1152), "club3.fc.bias": (2,),
            "RCNN_rpn.RPN_Conv.weight": (512, 512, 3, 3), "RCNN_cls_score.weight": (9, 4096)}
    for k, shape in want.items():
        assert k in sd and tuple(sd[k].shape) == shape, (k, sd.get(k, torch.empty(0)).shape)
    assert not [k for k in sd if k.startswith(("RCNN_rpn_t.", "align", "consistency"))]
    for view in ("conv3_s.", "conv3_t.", "conv34_s.", "conv34_t.", "conv45_s.", "conv45_t."):
        assert [k for k in sd if k.startswith(view)], view      # the views of the two stacks
    # the views count from 0 as the reference's fresh Sequentials do, and name the stacks' tensors
    assert sd["conv34_s.1.weight"].data_ptr() == sd["RCNN_base.17.weight"].data_ptr()
    assert sd["conv45_t.3.weight"].data_ptr() == sd["RCNN_base_t.26.weight"].data_ptr()
    assert sorted(k for k in sd if k.startswith("conv34_t.")) == \
        [f"conv34_t.{i}.{p}" for i in (1, 3, 5) for p in ("bias", "weight")]
    assert "RCNN_imageDA_3.Conv1.bias" not in sd and "RCNN_imageDA.Conv2.bias" not in sd
    # the frozen prefix is one set of tensors under both stacks' keys; the rest is copied
    assert sd["RCNN_base.0.weight"].data_ptr() == sd["RCNN_base_t.0.weight"].data_ptr()
    assert sd["RCNN_base.10.weight"].data_ptr() != sd["RCNN_base_t.10.weight"].data_ptr()
    for head in (m.RCNN_imageDA_3, m.RCNN_imageDA_4, m.RCNN_imageDA):
        assert isinstance(head.Convm1, StridedConv2d) and head.Convm1.stride == (3, 3)
        assert isinstance(head.Convm2, StridedConv2d) and head.Convm2.stride == (2, 2)
        assert isinstance(head.Conv1, Conv2d) and head.Conv1.relu and head.Convm1.relu
    for club in (m.club3, m.club4, m.club5):
        assert isinstance(club.out_score[0], StridedConv2d) and isinstance(club.out_score[2], Conv2d)
    assert default_clip(m) == 10.0
    # PyTorch's default init on the DA and CLUB modules: kaiming_uniform(a = sqrt(5)) bounds
    w = m.club4.out_score[0].weight.detach()
    assert float(w.abs().max()) <= 1.0 / (1024 * 9) ** 0.5 + 1e-7 < 0.011
    o = OraclePAATF(dropout=0.0)
    o.load_from(m)
    assert {k for k, p in o.named_parameters() if p.requires_grad} == \
        {k for k, p in m.named_parameters() if p.requires_grad}


def test_total_loss_weights():
    from tlod.da.pa_atf import vgg16
    s = [torch.tensor(float(v)) for v in (2, 3, 5, 7, 11, 13, 17, 19, 23)]
    rpn_c, rpn_b, rc, rb, da_img, t_da_img, da_ins, t_da_ins, pm = s
    out = (None, None, None, rpn_c, rpn_b, rc, rb, None, da_img, t_da_img, da_ins, t_da_ins, pm)
    det, da = 2 + 3 + 5 + 7, 11 + 13 + 17 + 19
    assert abs(float(vgg16.total_loss(out)) - (det + 0.1 * da + 0.1 * 23)) < 1e-5
    assert abs(float(vgg16.total_loss(out, 0.1, 0.5)) - (det + 0.1 * da + 0.5 * 23)) < 1e-5
    assert abs(float(vgg16.total_loss(out, 1.0)) - (det + da + 0.1 * 23)) < 1e-5


def test_forward_needs_the_target_in_training():
    from tlod.detector.train import build_model
    m = build_model("pa_atf", "cpu")
    with pytest.raises(RuntimeError, match="10-argument"):
        m(*[torch.zeros(1)] * 4)


# ---------------------------------------------------------------- StridedConv2d
def test_strided_conv2d_is_an_nn_conv2d():
    from tlod.conv import Conv2d, StridedConv2d, conv_out_size
    torch.manual_seed(0)
    m = StridedConv2d(6, 4, 5, stride=3, relu=True)
    torch.manual_seed(0)
    r = nn.Conv2d(6, 4, 5, stride=3)
    assert isinstance(m, nn.Conv2d) and not isinstance(m, Conv2d)
    assert list(m.state_dict()) == list(r.state_dict()) == ["weight", "bias"]
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), r.state_dict().values()))
    assert m.stride == (3, 3) and m.padding == (0, 0) and m.act_tap is None
    assert "relu=True" in repr(m)
    assert "bias" not in StridedConv2d(6, 4, 3, stride=2, padding=1, bias=False).state_dict()
    assert conv_out_size(20, 22, 5, 3, 0) == (6, 6) and conv_out_size(3, 3, 3, 2, 0) == (1, 1)
    assert conv_out_size(9, 11, 3, 2, 1) == (5, 6)
    with pytest.raises(NotImplementedError):
        StridedConv2d(6, 4, (3, 5))
    with pytest.raises(NotImplementedError):
        StridedConv2d(6, 4, 3, stride=(2, 1))
    with pytest.raises(NotImplementedError):
        StridedConv2d(6, 4, 3, stride=0)


def test_strided_conv2d_switch_off_runs_on_the_cpu(monkeypatch):
    from tlod.conv import StridedConv2d
    torch.manual_seed(1)
    m = StridedConv2d(6, 4, 5, stride=3, relu=True)
    x = torch.randn(2, 6, 23, 31)
    with pytest.raises(RuntimeError, match="MI355X only"):
        m(x)                                         # no quiet fall-back when the switch is on
    monkeypatch.setenv("TLOD_SCONV", "0")
    m.act_tap = []
    y = m(x)
    assert torch.equal(y, F.relu(F.conv2d(x, m.weight, m.bias, 3)))
    assert len(m.act_tap) == 1 and torch.equal(m.act_tap[0], y)


# ---------------------------------------------------------------- torch compositions
def test_gate_composition_is_the_reference_formula():
    """faster_rcnn.py:89 of the reference: sigmoid(adaptive_max_pool2d(z, (1, 1)))."""
    from tlod.da import pa_atf
    torch.manual_seed(2)
    z = torch.randn(2, 7, 3, 6, dtype=torch.float64, requires_grad=True)
    mask, arg = pa_atf.gate_torch(z)
    assert torch.equal(mask, torch.sigmoid(F.adaptive_max_pool2d(z, (1, 1))))
    assert arg.dtype == torch.int32 and tuple(arg.shape) == (2, 7)
    assert torch.equal(arg.long(), z.detach().view(2, 7, -1).argmax(2))
    mask.sum().backward()
    hit = z.grad.view(14, -1)
    assert int((hit != 0).sum()) == 14
    m = mask.detach().view(-1)
    assert torch.allclose(hit[torch.arange(14), arg.view(-1).long()], m * (1 - m), rtol=1e-12)
    assert pa_atf.fused_pa_atf()


def test_loss_compositions_are_the_reference_formulas():
    """The (R, R) broadcast of torch.abs(x (R, 1) - label (R)).mean() in closed form, the
    elementwise BCE with its clamp at -100, and the two-logit cross entropy."""
    from tlod.da import pa_atf
    torch.manual_seed(3)
    img = [torch.randn(2, 1, 3, 5, dtype=torch.float64) * 3 for _ in range(6)]
    img[0].view(-1)[0] = -200.0
    ins = [torch.randn(300, 1, dtype=torch.float64) for _ in range(2)]
    club = [torch.randn(4, 2, dtype=torch.float64) for _ in range(6)]
    out = pa_atf.losses_torch(img, [1, 1, 1, 0, 0, 0], ins, [256, 300], club, [1, 0] * 3)
    assert tuple(out.shape) == (14,)
    p = torch.sigmoid(img[0]).view(-1)
    assert abs(float(out[0]) - float((-torch.log(p).clamp(min=-100)).mean())) < 1e-12
    assert float(out[0]) > 100.0 / 30
    p = torch.sigmoid(img[3]).view(-1)
    assert abs(float(out[3]) - float((-torch.log(1 - p)).mean())) < 1e-12
    x = torch.sigmoid(ins[0])                                   # 256 ones, 44 zeros
    label = torch.cat((torch.ones(256), torch.zeros(44))).double()
    assert abs(float(out[6]) - float(torch.abs(x - label).mean())) < 1e-15
    closed = ((256 * (1 - x) + 44 * x) / 300).mean()
    assert abs(float(out[6]) - float(closed)) < 1e-12
    assert abs(float(out[7]) - float((1 - torch.sigmoid(ins[1])).mean())) < 1e-12   # constant label
    assert abs(float(out[9]) - float(F.cross_entropy(club[1], torch.zeros(4).long()))) < 1e-12
    with pytest.raises(ValueError):
        pa_atf.losses(img[:5], [1] * 5, ins, [0, 0], club, [1, 0] * 3)


def test_club_composition_is_the_reference_formula():
    """lib/PA_ATF/faster_rcnn.py:387-406 with CLUB.forward (:125-147), literally — plain
    nn.Conv2d / nn.Linear, torch.cat, nll_loss(log_softmax) and the two gradient reversals —
    against tlod.da.pa_atf: proto_pool_torch over a CPU RoI pool (oracle.roi), the CLUB module's
    plain statement and losses_torch.  Values and the gradient that reaches the pooled
    features, in fp64."""
    import numpy as np
    from oracle import roi as oroi
    from tlod.da import pa_atf
    torch.manual_seed(4)
    C, H, W, G, scale = 6, 12, 14, 3, 1 / 4
    feat = torch.randn(1, C, H, W)
    rois = torch.tensor([[0, 4.0, 6.0, 40.0, 39.0], [0, 10.0, 2.0, 52.0, 30.0],
                         [0, 20.0, 20.0, 21.0, 21.0]])
    pooled, _ = oroi.roi_pool_fwd(feat.numpy(), rois.numpy(), 7, 7, scale)
    cw = torch.rand(1, C, 1, 1, dtype=torch.float64, requires_grad=True)   # detached inside
    perm = torch.tensor([2, 0, 1])
    club = pa_atf.CLUB(C).double()
    assert list(club.state_dict()) == ["out_score.0.weight", "out_score.0.bias",
                                       "out_score.2.weight", "out_score.2.bias", "fc.weight",
                                       "fc.bias"]

    # the project's composition
    p1 = torch.from_numpy(pooled).double().requires_grad_(True)
    same, diff = pa_atf.proto_pool_torch(None, None, scale, cw, perm, 0.1, pooled=p1)
    assert tuple(same.shape) == tuple(diff.shape) == (G, 2 * C, 7, 7)
    z_same, z_diff = club.forward_torch(same, diff)
    dummy = [torch.zeros(1, 2, dtype=torch.float64)] * 4
    terms = pa_atf.losses_torch([], [], [], [], [z_same, z_diff] + dummy, [1, 0, 1, 0, 1, 0])
    got = terms[0] + terms[1]
    got.backward()

    # the reference's lines
    class GRL(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, alpha):
            ctx.alpha = alpha
            return x.view_as(x)

        @staticmethod
        def backward(ctx, g):
            return g.neg() * ctx.alpha, None
    out_score = nn.Sequential(nn.Conv2d(2 * C, C, kernel_size=3, stride=2), nn.ReLU(),
                              nn.Conv2d(C, 128, kernel_size=1, stride=1), nn.ReLU()).double()
    fc = nn.Linear(3 * 3 * 128, 2).double()
    out_score.load_state_dict({k[len("out_score."):]: v for k, v in club.state_dict().items()
                               if k.startswith("out_score.")})
    fc.load_state_dict({"weight": club.fc.weight.detach(), "bias": club.fc.bias.detach()})
    p2 = torch.from_numpy(pooled).double().requires_grad_(True)
    f_a, f_s = p2 * cw.detach(), p2 * (1 - cw.detach())
    x11, x22 = GRL.apply(f_a, 0.1), GRL.apply(f_s, 0.1)
    x22_r = x22[perm, :, :, :]
    same_conv = out_score(torch.cat((x11, x22), dim=1))
    diff_conv = out_score(torch.cat((x11, x22_r), dim=1))
    same_prob = F.log_softmax(fc(same_conv.view(G, -1)), dim=1)
    diff_prob = F.log_softmax(fc(diff_conv.view(G, -1)), dim=1)
    want = F.nll_loss(same_prob, torch.ones(G).long()) + F.nll_loss(diff_prob, torch.zeros(G).long())
    want.backward()
    assert abs(float(got.detach()) - float(want.detach())) < 1e-12
    assert float(p2.grad.abs().max()) > 0
    assert torch.allclose(p1.grad, p2.grad, rtol=1e-10, atol=1e-14)
    assert cw.grad is None                                     # the mask is detached
    for a, b in zip(club.parameters(), list(out_score.parameters()) + list(fc.parameters())):
        assert torch.allclose(a.grad, b.grad, rtol=1e-10, atol=1e-14)
    # the reversal: without it the gradient would be -10 times this one
    p3 = torch.from_numpy(pooled).double().requires_grad_(True)
    a3 = p3 * cw.detach()
    plain = out_score(torch.cat((a3, p3 * (1 - cw.detach())), dim=1))
    F.nll_loss(F.log_softmax(fc(plain.view(G, -1)), dim=1), torch.ones(G).long()).backward()
    club.zero_grad()
    p4 = torch.from_numpy(pooled).double().requires_grad_(True)
    s4, d4 = pa_atf.proto_pool_torch(None, None, scale, cw, perm, 0.1, pooled=p4)
    z4, _ = club.forward_torch(s4, d4)
    F.nll_loss(F.log_softmax(z4, 1), torch.ones(G).long()).backward()
    assert torch.allclose(p4.grad, -0.1 * p3.grad, rtol=1e-10, atol=1e-14)
    assert np.isfinite(float(got.detach()))
