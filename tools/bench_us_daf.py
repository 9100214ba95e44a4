"""Step time of US-DAF beside DAF (synthetic Cityscapes -> Foggy batches), one session.

Per backbone (VGG16 and ResNet101) three figures, interleaved over --rounds rounds so drift
hits them alike:
  daf              tlod.detector.train.train_step on a DAF model (the yardstick: US-DAF does a
                   subset of DAF's domain work, it has no consistency terms)
  us_daf           the same step on a US-DAF model, fused ops
  us_daf_unfused   the same step with TLOD_FUSED_LOSSES=0: the torch compositions of the scale
                   labels, sigmoids and BCE terms (and of the RPN / RCNN losses, which the
                   switch also covers)
Each timed step is bracketed by device events after --warmup untimed steps of its own
configuration; a figure is the median over its timed steps (mean and min beside it), and
"round_medians" lists the median of each round: their range is the run-to-run spread.

  python tools/bench_us_daf.py --steps 50 --warmup 10 --rounds 3 --out profiles/us_daf/step_times.txt
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "transfer-learning-library-for-object-detection_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--nets", default="vgg16,res101")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch
    from tlod.detector.train import SyntheticCityscapes, build_model, make_optimizer, train_step
    if not torch.cuda.is_available():
        raise SystemExit("bench_us_daf.py measures on the MI355X: no GPU here")
    dev = torch.device("cuda:0")
    data = SyntheticCityscapes(dev, H=args.height, W=args.width)
    lines = []
    for net in args.nets.split(","):
        models = {}
        for method in ("daf", "us_daf"):
            m = build_model(method, dev, net)
            models[method] = (m, make_optimizer(m, 2e-3))
        configs = [("daf", "daf", "1"), ("us_daf", "us_daf", "1"), ("us_daf_unfused", "us_daf", "0")]
        times = {name: [] for name, _, _ in configs}
        rounds = {name: [] for name, _, _ in configs}
        for _ in range(args.rounds):
            for name, method, fused in configs:
                m, opt = models[method]
                os.environ["TLOD_FUSED_LOSSES"] = fused
                for _ in range(args.warmup):
                    train_step(m, opt, data.next())
                torch.cuda.synchronize()
                events = []
                for _ in range(args.steps):
                    t0 = torch.cuda.Event(enable_timing=True)
                    t1 = torch.cuda.Event(enable_timing=True)
                    t0.record()
                    loss = train_step(m, opt, data.next())
                    t1.record()
                    events.append((t0, t1))
                torch.cuda.synchronize()
                assert torch.isfinite(loss), (net, name, float(loss))
                t = [a.elapsed_time(b) for a, b in events]
                times[name] += t
                rounds[name].append(round(statistics.median(t), 3))
        os.environ.pop("TLOD_FUSED_LOSSES", None)
        for name, _, _ in configs:
            t = times[name]
            lines.append(json.dumps({
                "net": net, "config": name, "H": args.height, "W": args.width, "steps": len(t),
                "ms_per_step_median": round(statistics.median(t), 3),
                "ms_per_step_mean": round(statistics.fmean(t), 3),
                "ms_per_step_min": round(min(t), 3), "round_medians": rounds[name]}))
            print(lines[-1], flush=True)
        del models
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
