"""Step time of IDF-VGG16 beside DAF-VGG16 (synthetic Cityscapes -> Foggy batches, 600x1200),
one session on one MI355X.

Three figures, interleaved over --rounds rounds so drift hits them alike:
  daf           tlod.detector.train.train_step on a DAF-VGG16 model (the yardstick of a step on
                this chip; its round-to-round range is the run-to-run spread)
  idf           tlod.detector.train.idf_train_step, fused DAM / separation / domain-loss kernels
  idf_unfused   the same step with TLOD_FUSED_IDF=0: the torch compositions of the same math
Each timed step is bracketed by device events after --warmup untimed steps of its own
configuration; a figure is the median over its timed steps (mean and min beside it), and
"round_medians" lists the median of each round.

A fourth line, "idf_discriminators", is the share of the step spent in the seven discriminator
trunks (torch modules: 1x1 / strided 3x3 convs, batch norm, dropout), forward and backward:
the fused IDF step's forward + backward timed with the trunks swapped for stubs and the domain
terms left out of the loss is subtracted from the full forward + backward (no optimizer step
in either).

  python tools/bench_idf.py --steps 30 --warmup 8 --rounds 3 --out profiles/idf/step_times.txt
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "transfer-learning-library-for-object-detection_amd")]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch
    from tlod.detector.train import (SyntheticCityscapes, build_model, idf_forward,
                                     idf_train_step, make_optimizer, train_step)
    if not torch.cuda.is_available():
        raise SystemExit("bench_idf.py measures on the MI355X: no GPU here")
    dev = torch.device("cuda:0")
    data = SyntheticCityscapes(dev, H=args.height, W=args.width)
    pseudo = SyntheticCityscapes(dev, H=args.height, W=args.width, tgt_G=8)
    daf = build_model("daf", dev)
    daf_opt = make_optimizer(daf, 2e-3)
    idf = build_model("idf", dev)
    # a step's time does not depend on the learning rate; IDF has no gradient clipping, and a
    # randomly initialised model (the pretrained weights are external) diverges within a few
    # dozen steps at DAF's 2e-3, so the timed updates are kept small
    idf_opt = make_optimizer(idf, 1e-6)

    def idf_fwd_bwd(heads):
        """Forward + backward of the IDF step without the update; heads=False leaves the
        domain terms out of the loss (the discriminators are then swapped for stubs below)."""
        idf_opt.zero_grad(set_to_none=True)
        out_s, out_t = idf_forward(idf, pseudo.next(), True)
        if heads:
            loss = idf.total_loss(out_s, out_t, True, 3.0)
        else:
            loss = sum(out_s[3:7]) + 0.5 * sum(out_t[3:7]) + out_s[15] + out_s[16] + out_t[15] \
                + out_t[16]
        loss.backward()
        return loss.detach()

    configs = [
        ("daf", "1", lambda: train_step(daf, daf_opt, data.next())),
        ("idf", "1", lambda: idf_train_step(idf, idf_opt, pseudo.next())),
        ("idf_unfused", "0", lambda: idf_train_step(idf, idf_opt, pseudo.next())),
        ("idf_fwd_bwd", "1", lambda: idf_fwd_bwd(True)),
    ]
    times = {name: [] for name, _, _ in configs}
    rounds = {name: [] for name, _, _ in configs}
    for _ in range(args.rounds):
        for name, fused, fn in configs:
            os.environ["TLOD_FUSED_IDF"] = fused
            t = timed(fn, args.steps, args.warmup)
            times[name] += t
            rounds[name].append(round(statistics.median(t), 3))
    os.environ.pop("TLOD_FUSED_IDF", None)

    # the discriminators' share: the same forward + backward with the trunks out of the graph
    class _Skip(torch.nn.Module):
        def __init__(self, rows):
            super().__init__()
            self.rows = rows

        def forward(self, x):
            return x.new_zeros((x.shape[0] if self.rows else 1, 2))

    names = ("netD_1", "netD_2", "netD_3", "netD_1_b", "netD_2_b", "netD_3_b", "netD_da")
    kept = {n: getattr(idf, n) for n in names}
    for n in names:
        setattr(idf, n, _Skip(n == "netD_da"))
    bare = timed(lambda: idf_fwd_bwd(False), args.steps * args.rounds, args.warmup)
    for n in names:
        setattr(idf, n, kept[n])

    lines = []
    for name, _, _ in configs:
        t = times[name]
        lines.append(json.dumps({
            "net": "vgg16", "config": name, "H": args.height, "W": args.width, "steps": len(t),
            "ms_per_step_median": round(statistics.median(t), 3),
            "ms_per_step_mean": round(statistics.fmean(t), 3),
            "ms_per_step_min": round(min(t), 3), "round_medians": rounds[name]}))
    full, none = statistics.median(times["idf_fwd_bwd"]), statistics.median(bare)
    lines.append(json.dumps({
        "net": "vgg16", "config": "idf_discriminators", "H": args.height, "W": args.width,
        "fwd_bwd_ms_with": round(full, 3), "fwd_bwd_ms_without": round(none, 3),
        "ms_per_step": round(full - none, 3),
        "share_of_idf_step": round((full - none) / statistics.median(times["idf"]), 3)}))
    for line in lines:
        print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
