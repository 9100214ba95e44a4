"""Step time of PT-MAF beside MAF (VGG16, synthetic Cityscapes -> Foggy batches), one session.

Three figures, interleaved over --rounds rounds so drift hits them alike:
  maf              tlod.detector.train.train_step on a MAF model
  pt_maf           pt_maf_train_step (student + frozen teacher + KD), fused ops
  pt_maf_unfused   the same step with TLOD_FUSED_LOSSES=0: the torch compositions of the
                   maps, the masked NLLs and the KD sums (and of the RPN loss, which the
                   switch also covers)
Each timed step is bracketed by device events after --warmup untimed steps of its own
configuration; a figure is the median over its timed steps (mean and min beside it).  The gt
cell mask has no torch composition without a host loop, so both PT-MAF figures use the kernel.

  python tools/bench_pt_maf.py --steps 20 --warmup 5 --rounds 2
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--width", type=int, default=1200)
    args = ap.parse_args()

    import torch
    from tlod.detector.train import (SyntheticCityscapes, build_model, make_optimizer,
                                     pt_maf_train_step, train_step)
    if not torch.cuda.is_available():
        raise SystemExit("bench_pt_maf.py measures on the MI355X: no GPU here")
    dev = torch.device("cuda:0")
    data = SyntheticCityscapes(dev, H=args.height, W=args.width)
    maf = build_model("maf", dev)
    maf_opt = make_optimizer(maf, 2e-3)
    student = build_model("pt_maf", dev)
    student_opt = make_optimizer(student, 2e-3)
    teacher = build_model("faster_rcnn", dev, seed=1).eval()

    def pt_step():
        return pt_maf_train_step(student, teacher, student_opt, data.next())

    configs = [("maf", "1", lambda: train_step(maf, maf_opt, data.next())),
               ("pt_maf", "1", pt_step), ("pt_maf_unfused", "0", pt_step)]
    times = {name: [] for name, _, _ in configs}
    for _ in range(args.rounds):
        for name, fused, step in configs:
            os.environ["TLOD_FUSED_LOSSES"] = fused
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            events = []
            for _ in range(args.steps):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                loss = step()
                t1.record()
                events.append((t0, t1))
            torch.cuda.synchronize()
            assert torch.isfinite(loss), (name, float(loss))
            times[name] += [a.elapsed_time(b) for a, b in events]
    os.environ.pop("TLOD_FUSED_LOSSES", None)
    for name, _, _ in configs:
        t = times[name]
        print(json.dumps({"config": name, "H": args.height, "W": args.width,
                          "steps": len(t), "ms_per_step_median": round(statistics.median(t), 3),
                          "ms_per_step_mean": round(statistics.fmean(t), 3),
                          "ms_per_step_min": round(min(t), 3)}))


if __name__ == "__main__":
    main()
