"""Step time of PA-ATF-VGG16 beside DAF- and ATF-VGG16 (synthetic Cityscapes -> Foggy batches,
600x1200), and StridedConv2d beside F.conv2d on PA-ATF's, CLUB's and IDF's shapes; one session
on one MI355X.

Step figures, interleaved over --rounds rounds so drift hits them alike:
  daf             tlod.detector.train.train_step on a DAF-VGG16 model (the yardstick of a step
                  on this chip; its round-to-round range is the run-to-run spread)
  atf             the same on ATF-VGG16, the method PA-ATF extends
  pa_atf          PA-ATF, every switch on
  pa_atf_unfused  TLOD_FUSED_PA_ATF=0: the torch compositions of the gate, the prototype pooling
                  and the 14 loss terms
  pa_atf_sconv0   TLOD_SCONV=0: the strided convolutions on F.conv2d
Each timed step is bracketed by device events after --warmup untimed steps of its own
configuration; a figure is the median over its timed steps (mean and min beside it), and
"round_medians" lists the median of each round.  A switch earns its default only if its
pa_atf median beats the switched-off median by more than the daf spread of the same session.

Op figures (--ops): forward + backward of one strided convolution (input, weight and bias
gradients), median of event-timed calls, StridedConv2d against F.conv2d on the same tensors:
the six mask-net shapes and CLUB's three at 600x1200 with 8 gt boxes, and IDF's 3x3 stride-2
pad-1 discriminator trunk shapes.

  python tools/bench_pa_atf.py --steps 20 --warmup 5 --rounds 3 --ops \
      --out profiles/pa_atf/step_times.txt --ops-out profiles/pa_atf/sconv_ops.txt
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "transfer-learning-library-for-object-detection_amd")]

SWITCHES = ("TLOD_FUSED_PA_ATF", "TLOD_SCONV")

# (name, N, Cin, H, W, KS, stride, pad, Cout, relu) at 600x1200: conv3 150x300, conv4 75x150,
# conv5 37x75; Convm2 reads the 2x2 max-pool of Convm1's output
OP_SHAPES = [
    ("ida3.Convm1", 2, 256, 150, 300, 5, 3, 0, 256, True),
    ("ida3.Convm2", 2, 256, 24, 49, 3, 2, 0, 256, False),
    ("ida4.Convm1", 2, 512, 75, 150, 5, 3, 0, 512, True),
    ("ida4.Convm2", 2, 512, 12, 24, 3, 2, 0, 512, False),
    ("ida5.Convm1", 2, 512, 37, 75, 5, 3, 0, 512, True),
    ("ida5.Convm2", 2, 512, 5, 12, 3, 2, 0, 512, False),
    ("club3.out_score.0", 16, 512, 7, 7, 3, 2, 0, 256, True),
    ("club4.out_score.0", 16, 1024, 7, 7, 3, 2, 0, 512, True),
    ("club5.out_score.0", 16, 1024, 7, 7, 3, 2, 0, 512, True),
    ("idf.netD_2.conv1", 1, 512, 75, 150, 3, 2, 1, 512, False),
    ("idf.netD_2.conv2", 1, 512, 38, 75, 3, 2, 1, 128, False),
    ("idf.netD_3.conv1", 1, 512, 37, 75, 3, 2, 1, 512, False),
    ("idf.netD_3.conv2", 1, 512, 19, 38, 3, 2, 1, 128, False),
]


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    events = []
    for _ in range(steps):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        events.append((t0, t1))
    torch.cuda.synchronize()
    assert out is None or torch.isfinite(out), float(out)
    return [a.elapsed_time(b) for a, b in events]


def op_table(dev, steps, warmup):
    import torch
    from tlod.conv import StridedConv2d
    lines = []
    for name, N, C, H, W, KS, s, p, Cout, relu in OP_SHAPES:
        m = StridedConv2d(C, Cout, KS, stride=s, padding=p, relu=relu).to(dev)
        x = torch.randn(N, C, H, W, device=dev, requires_grad=True)
        row = {"op": name, "N": N, "Cin": C, "H": H, "W": W, "KS": KS, "stride": s, "pad": p,
               "Cout": Cout}

        def fwd_bwd():
            x.grad = None
            m.zero_grad(set_to_none=True)
            m(x).sum().backward()
        for key, flag in (("sconv_ms", "1"), ("f_conv2d_ms", "0")):
            os.environ["TLOD_SCONV"] = flag
            row[key] = round(statistics.median(timed(fwd_bwd, steps, warmup)), 4)
        os.environ.pop("TLOD_SCONV", None)
        Ho, Wo = (H + 2 * p - KS) // s + 1, (W + 2 * p - KS) // s + 1
        row["gflop_fwd_bwd"] = round(3 * 2.0 * N * Ho * Wo * Cout * C * KS * KS / 1e9, 2)
        lines.append(json.dumps(row))
        del m, x
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--ops", action="store_true", help="also time the op-level table")
    ap.add_argument("--out", default=None, help="also append the step JSON lines to this file")
    ap.add_argument("--ops-out", default=None, help="also append the op JSON lines to this file")
    args = ap.parse_args()

    import torch
    from tlod.detector.train import SyntheticCityscapes, build_model, make_optimizer, train_step
    if not torch.cuda.is_available():
        raise SystemExit("bench_pa_atf.py measures on the MI355X: no GPU here")
    dev = torch.device("cuda:0")
    data = SyntheticCityscapes(dev, H=args.height, W=args.width)
    models = {k: build_model(k, dev) for k in ("daf", "atf", "pa_atf")}
    opts = {k: make_optimizer(m, 2e-3 if k != "pa_atf" else 1e-4) for k, m in models.items()}

    def step(k):
        return lambda: train_step(models[k], opts[k], data.next())
    configs = [("daf", {}, step("daf")), ("atf", {}, step("atf")), ("pa_atf", {}, step("pa_atf")),
               ("pa_atf_unfused", {"TLOD_FUSED_PA_ATF": "0"}, step("pa_atf")),
               ("pa_atf_sconv0", {"TLOD_SCONV": "0"}, step("pa_atf"))]
    times = {name: [] for name, _, _ in configs}
    rounds = {name: [] for name, _, _ in configs}
    for _ in range(args.rounds):
        for name, env, fn in configs:
            for k in SWITCHES:
                os.environ[k] = env.get(k, "1")
            t = timed(fn, args.steps, args.warmup)
            times[name] += t
            rounds[name].append(round(statistics.median(t), 3))
    for k in SWITCHES:
        os.environ.pop(k, None)

    lines = []
    for name, _, _ in configs:
        t = times[name]
        lines.append(json.dumps({
            "net": "vgg16", "config": name, "H": args.height, "W": args.width, "steps": len(t),
            "ms_per_step_median": round(statistics.median(t), 3),
            "ms_per_step_mean": round(statistics.fmean(t), 3),
            "ms_per_step_min": round(min(t), 3), "round_medians": rounds[name]}))
    spread = max(rounds["daf"]) - min(rounds["daf"])
    med = {k: statistics.median(v) for k, v in times.items()}
    lines.append(json.dumps({
        "config": "decision", "daf_spread_ms": round(spread, 3),
        "fused_gain_ms": round(med["pa_atf_unfused"] - med["pa_atf"], 3),
        "sconv_gain_ms": round(med["pa_atf_sconv0"] - med["pa_atf"], 3)}))
    for line in lines:
        print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    if args.ops:
        del models, opts
        torch.cuda.empty_cache()
        ops = op_table(dev, max(args.steps, 10), args.warmup)
        for line in ops:
            print(line, flush=True)
        if args.ops_out:
            os.makedirs(os.path.dirname(os.path.abspath(args.ops_out)), exist_ok=True)
            with open(args.ops_out, "a") as f:
                f.write("\n".join(ops) + "\n")


if __name__ == "__main__":
    main()
