"""Throughput benchmark of the DAF VGG16 Cityscapes->Foggy training step on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    (N > 1: python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...)

One step = one DAF iteration on one source + one target image (600x1200, synthetic,
resident in HBM) per GPU: forward, loss, backward (+ RCCL gradient all-reduce for N>1),
clip_gradient(10), SGD.  value = source images/s over the whole job (max-over-ranks
step time).  Rank 0 prints one JSON line.

A plain run sets up, warms up, times the K steps and prints the line (roofline and
cpu_baseline are null).  --full adds the per-launch conv / GEMM roofline (one untimed
launch-counting step before the timed region, HIP events on its last step, the committed
PMC traffic) and the CPU baseline of the oracle step; see DESIGN.md §Measurement for
those fields.  --dump-outputs DIR writes what the last timed step handed back (its loss,
the losses of all timed steps, a fixed sample of every updated parameter) as
DIR/<name>.npy; the inputs depend on the arguments only, so two builds compare file by file.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "transfer-learning-library-for-object-detection_amd")
for _p in (ROOT, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

METRIC = ("training images/sec (whole node) DAF VGG16 Cityscapes→Foggy, bs=1/img/GPU at "
          "1/2/4/8 MI355X")
F32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
BF16_MFMA_PEAK_TFLOPS = 2516.6  # v_mfma_f32_32x32x16_bf16: 1024 flop/clk/SIMD x 1024 SIMDs x 2.4 GHz
# f32-equivalent peak of each conv arithmetic (algorithmic f32 FLOPs per second at MFMA peak):
# the split-bf16 paths issue 6 (3) bf16 products per f32 product
PEAKS = {"f32": F32_MFMA_PEAK_TFLOPS, "bf16x6": BF16_MFMA_PEAK_TFLOPS / 6,
         "bf16x3": BF16_MFMA_PEAK_TFLOPS / 3}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--full", action="store_true",
                    help="also measure the conv / GEMM roofline (per-launch events) and the "
                         "CPU baseline; a plain run only times the steps")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as DIR/<name>.npy "
                         "(float32 / float64)")
    ap.add_argument("--cpu-baseline-steps", type=int, default=5,
                    help="--full: oracle CPU steps timed on rank 0 at N=1, after 2 untimed "
                         "(0 disables)")
    ap.add_argument("--cpu-threads", type=int, default=16,
                    help="torch CPU threads of the baseline (the box's share of one GPU is 16)")
    ap.add_argument("--bucket-mb", type=float, default=32.0)
    ap.add_argument("--net", choices=("vgg16", "res101"), default="vgg16")
    ap.add_argument("--classes", type=int, choices=(9, 21), default=None,
                    help="9: Cityscapes (default), 21: PASCAL VOC (default for --method atf: "
                         "BASELINE config 5, PASCAL->Clipart)")
    ap.add_argument("--method", choices=("daf", "maf", "atf"), default="daf",
                    help="detector (the headline metric is DAF; MAF / ATF are secondary workloads)")
    return ap.parse_args()


def conv_bytes(kind, shape):
    """Algorithmic HBM bytes of one launch: each operand read once, the result written once
    (fp32).  Convs: shape = (N, Cin, H, W, Cout, KS) of the forward convolution; GEMMs
    (tlod.linear): shape = (M, N, K)."""
    if kind.startswith("gemm"):
        M, N, K = shape
        return 4 * (M * K + N * K + M * N)
    N, Cin, H, W, Cout, KS = shape
    x, y, w = N * Cin * H * W * 4, N * Cout * H * W * 4, Cout * Cin * KS * KS * 4
    return x + y + w  # fwd: X, W -> Y; dgrad: dY, W -> dX; wgrad: dY, X -> dW


def family(kind, shape):
    """Kernel family of a timed launch: (op, arithmetic) — op conv3x3 (the patch-staged and
    warp-specialized kernels), conv1x1 (the per-image conv GEMM) or gemm (tlod.linear's
    fc / RoI-head GEMMs)."""
    math = kind.split("/")[1]
    if kind.startswith("gemm"):
        return "gemm/" + math
    return ("conv3x3/" if shape[5] == 3 else "conv1x1/") + math


def conv_roofline(records):
    """Aggregate the timed conv and GEMM launches: algorithmic FLOPs / measured kernel time,
    per kind and per family; the dominant family is the one with the most time."""
    tot_f, tot_ms, by, shapes, fam = 0.0, 0.0, {}, {}, {}
    for s, e, flops, kind, shape in records:
        ms = s.elapsed_time(e)
        tot_f += flops
        tot_ms += ms
        for key, table in ((kind, by), ((kind,) + tuple(shape), shapes),
                           (family(kind, shape), fam)):
            d = table.setdefault(key, [0.0, 0.0, 0, 0.0])
            d[0] += flops
            d[1] += ms
            d[2] += 1
            d[3] += conv_bytes(kind, shape)
    if os.environ.get("TLOD_BENCH_SHAPES"):
        for k, v in sorted(shapes.items(), key=lambda kv: -kv[1][1]):
            print(f"{k[0]:12s} {k[1:]} launches={v[2]:4d} ms={v[1]:8.3f} "
                  f"TF={v[0] / (v[1] * 1e-3) / 1e12:7.2f}", file=sys.stderr)
    if tot_ms == 0:
        return 0.0, {}, 0.0, 0.0, 0, None, {}
    achieved = tot_f / (tot_ms * 1e-3) / 1e12
    detail = {k: {"launches": v[2], "ms": round(v[1], 3),
                  "tflops": round(v[0] / (v[1] * 1e-3) / 1e12, 2),
                  "peak": round(PEAKS[k.split("/")[1]], 1)} for k, v in by.items()}
    fams = {k: {"launches": v[2], "ms": round(v[1], 3),
                "tflops": round(v[0] / (v[1] * 1e-3) / 1e12, 2),
                "frac": round(v[0] / (v[1] * 1e-3) / 1e12 / PEAKS[k.split("/")[1]], 4)}
            for k, v in fam.items()}
    # the dominant kernel family (most time): its own achieved / peak
    dom = max(fam, key=lambda m: fam[m][1])
    dominant = {"family": dom, "math": dom.split("/")[1],
                "achieved": fam[dom][0] / (fam[dom][1] * 1e-3) / 1e12,
                "peak": PEAKS[dom.split("/")[1]], "ms": fam[dom][1], "launches": fam[dom][2],
                "bytes": fam[dom][3]}
    return achieved, detail, tot_ms, tot_f, len(records), dominant, fams


def measured_traffic(a):
    """Per-kernel HBM bytes per step from the latest committed PMC passes of this same bench
    command (profiles/r*/traffic.json, tools/pmc_traffic.py: FETCH_SIZE x2 + WRITE_SIZE per
    kernel); None for workloads it was not measured on."""
    import glob
    if (a.method, a.net, a.height, a.width) != ("daf", "vgg16", 600, 1200):
        return None, None
    here = os.path.dirname(os.path.abspath(__file__))
    files = sorted(glob.glob(os.path.join(here, "profiles", "r*", "traffic.json")))
    if not files:
        return None, None
    with open(files[-1]) as f:
        return json.load(f), os.path.relpath(files[-1], here)


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(steps, H, W, threads):
    """The oracle's CPU DAF step (test-infrastructure restatement) on this host's cores:
    2 untimed + ``steps`` timed steps, the median."""
    import oracle.daf_step as ods
    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    threads = max(1, min(threads, avail))
    torch.set_num_threads(threads)
    t = ods.time_cpu_steps(steps, H, W, warmup=2)
    return {"value": round(1.0 / t, 4), "unit": "img/s", "cores": threads,
            "cores_available": avail,
            "cores_note": "BASELINE.md §2 asks for all of sched_getaffinity; the GPU box's share "
                          "of one GPU is 16 host cores, and the oracle step measured slower at "
                          "64 threads (0.20 img/s) than at 16 (0.36; DESIGN §5), so it runs on "
                          "min(16, available)",
            "kind": "port", "cpu_model": cpu_model(),
            "sample": f"2 untimed + {steps} timed DAF-VGG16 steps (1 src + 1 tgt image {H}x{W}, "
                      f"synthetic) of the oracle restatement: numpy RPN/NMS/RoIAlign + torch-CPU "
                      f"fp32 conv/linear, {threads} threads; median s/step = {t:.2f}"}


def roofline_entry(a, records, n_prof):
    """The result line's roofline field (--full): the dominant kernel family of the timed
    conv + GEMM launches in ``records``, next to the committed PMC traffic."""
    achieved, detail, conv_ms, conv_f, n_launch, dom, fams = conv_roofline(records)
    if dom is None:  # TLOD_BENCH_NOPROF: no launch records
        dom = {"family": "none", "math": "bf16x6", "achieved": 0.0, "peak": 1.0, "ms": 0.0,
               "launches": 1, "bytes": 0.0}
    traffic, traffic_src = measured_traffic(a)
    fam_kernels = {"conv3x3/bf16x6": ("conv_fwd_bs_kernel", "conv_fwd_bs_ws_kernel",
                                      "wgrad_ws_kernel"),
                   "conv3x3/f32": ("conv_fwd_kernel", "conv_wgrad_kernel"),
                   "conv1x1/bf16x6": ("conv_gemm_bs_kernel", "conv_wgrad_bs_kernel"),
                   "gemm/bf16x6": ("gemm_bs_kernel",)}
    dom_kernels = fam_kernels.get(dom["family"], ())
    per_launch_pmc = None
    if traffic and dom_kernels:
        by_k = traffic["bytes_per_step_by_kernel"]
        # a PMC pass that predates a kernel of the family cannot price this run's launches
        if all(k in by_k for k in dom_kernels if k != "conv_fwd_bs_kernel"):
            per_launch_pmc = round(sum(by_k.get(k, 0) for k in dom_kernels) /
                                   (dom["launches"] / n_prof))
    return {"bound": "mfma", "achieved": round(dom["achieved"], 2),
            "peak": round(dom["peak"], 1), "unit": "TFLOP/s",
            "frac": round(dom["achieved"] / dom["peak"], 4),
            "traffic": per_launch_pmc,
            "algorithmic_bytes": round(dom["bytes"] / dom["launches"]),
            "traffic_source": traffic_src,
            "traffic_note": "PMC HBM bytes per launch of the dominant kernels "
                            f"({' + '.join(dom_kernels)}; FETCH_SIZE x2 + WRITE_SIZE) "
                            "vs algorithmic bytes per launch (operands read once, "
                            "result written once)" +
                            ("" if per_launch_pmc is not None or not traffic else
                             "; null: the committed PMC pass predates a kernel "
                             "of the family"),
            "traffic_by_kernel_per_step": (traffic or {}).get("bytes_per_step_by_kernel"),
            "kernel": f"tlod {dom['family']} (the family with the most time of "
                      "the timed conv + GEMM launches)",
            "kernel_ms_per_step": round(dom["ms"] / n_prof, 3),
            "profiled_steps": n_prof,
            "families": fams,
            "peak_basis": "f32-equivalent: algorithmic f32 FLOPs at the MFMA peak; "
                          "bf16xN = 2516.6 TF bf16 dense / N products",
            "all_conv_gemm": {"achieved": round(achieved, 2), "launches": n_launch,
                              "kernel_ms_per_step": round(conv_ms / n_prof, 3),
                              "gflop_per_step": round(conv_f / n_prof / 1e9, 2)},
            "by_kind": detail}


DUMP_BUDGET_BYTES = 48 << 20  # of the 64 MB a dump may take


def dump_outputs(out_dir, model, losses):
    """What a caller of train_step has after the last timed step: the loss it returned
    (loss.npy; losses.npy holds every timed step's) and the parameters it updated in place
    (param.<name>.npy).  A parameter larger than the per-tensor cap is written as a sample
    at fixed positions (seeded by the parameter's index and size only), so the files of two
    builds hold the same elements."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    all_losses = torch.stack(losses).double().reshape(-1).cpu().numpy()
    np.save(os.path.join(out_dir, "loss.npy"), all_losses[-1:])
    np.save(os.path.join(out_dir, "losses.npy"), all_losses)
    params = [(k, p.detach()) for k, p in model.named_parameters()]
    cap = 1 << 16
    while sum(min(p.numel(), cap) for _, p in params) * 4 > DUMP_BUDGET_BYTES:
        cap //= 2
    for i, (k, p) in enumerate(params):
        flat = p.reshape(-1)
        if flat.numel() > cap:
            rng = np.random.default_rng([i, flat.numel()])
            idx = np.sort(rng.integers(0, flat.numel(), cap))
            flat = flat[torch.from_numpy(idx).to(flat.device)]
        np.save(os.path.join(out_dir, f"param.{k}.npy"), flat.float().cpu().numpy())


def main():
    a = parse()
    from tlod.dist import GradBucketReducer, init_from_env
    from tlod import conv as tconv
    from tlod.linear import linear_math
    from tlod.detector.train import (SyntheticCityscapes, build_model, make_optimizer,
                                     train_step)

    # TLOD_DIST_BACKEND=gloo: the multi-rank path on one GPU (ranks share cuda:0) — a
    # plumbing rehearsal of the RCCL run, not a measurement
    rank, world = init_from_env(os.environ.get("TLOD_DIST_BACKEND"))
    local = int(os.environ.get("LOCAL_RANK", 0))
    if os.environ.get("TLOD_DIST_BACKEND") == "gloo":
        local = 0
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    ncls = a.classes or (21 if a.method == "atf" else 9)
    if ncls == 21:
        from tlod.data.imdb import VOC_CLASSES
        model = build_model(a.method, dev, a.net, classes=VOC_CLASSES, dataset="pascal_voc")
    else:
        model = build_model(a.method, dev, a.net)
    # clip_gradient(10) also for ResNet101 (the reference clips VGG16 only, DAF_train.py:406):
    # with random-init weights the unclipped first steps diverge; the fused step does the
    # same work either way (the norm is always computed)
    opt = make_optimizer(model, 2e-3, clip=10.0)
    reducer = GradBucketReducer(model, bucket_mb=a.bucket_mb) if world > 1 else None
    data = SyntheticCityscapes(dev, H=a.height, W=a.width, seed=1000 * rank + 1)

    for _ in range(a.warmup):
        train_step(model, opt, data.next(), reducer=reducer)
    torch.cuda.synchronize()

    class Records(list):
        """Per-launch (start, end) HIP event pairs of the timed region; the events are created
        beforehand (pool), so recording costs the host one hipEventRecord each."""
        pool = []

    # The per-launch events (--full) go on the LAST n_prof timed steps only
    # (TLOD_BENCH_PROF_STEPS, default 1): an event pair on every launch of every step took 3%
    # of the DAF-VGG16 step and 12% of the DAF-ResNet101 step (14.23 vs 13.81 ms, 21.47 vs
    # 18.87 ms, back to back) — each timing event is a stream marker the GPU stops for.
    n_prof = max(1, min(a.steps, int(os.environ.get("TLOD_BENCH_PROF_STEPS", "1"))))
    records = Records()
    if a.full:
        # launches per step, counted on one untimed step
        probe = Records()
        tconv.PROFILE = probe
        train_step(model, opt, data.next(), reducer=reducer)
        tconv.PROFILE = None
        torch.cuda.synchronize()
        records.pool = [(torch.cuda.Event(enable_timing=True),
                         torch.cuda.Event(enable_timing=True))
                        for _ in range(len(probe) * n_prof + 64)]
        del probe
    # a plain run, or TLOD_BENCH_NOPROF=1 under --full (diagnostic): no per-launch events
    # at all (no roofline)
    noprof = not a.full or os.environ.get("TLOD_BENCH_NOPROF") == "1"
    stats0 = dict(tconv.STATS)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    losses = []
    sync = os.environ.get("TLOD_BENCH_SYNC") == "1"  # A/B: host waits for every step
    for i in range(a.steps):
        if i == a.steps - n_prof and not noprof:
            tconv.PROFILE = records
        losses.append(train_step(model, opt, data.next(), reducer=reducer))
        if sync:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t1 = time.perf_counter()
    tconv.PROFILE = None
    elapsed = torch.tensor([t1 - t0], dtype=torch.float64, device=dev)
    per_rank = [float(elapsed.item())]
    if world > 1:
        gathered = [torch.zeros_like(elapsed) for _ in range(world)]
        dist.all_gather(gathered, elapsed)
        per_rank = [float(g.item()) for g in gathered]
        dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
    el = float(elapsed.item())
    ms_per_step = el / a.steps * 1e3
    value = world * a.steps / el  # one source image per rank per step
    last_loss = float(torch.stack(losses).float().mean().item())

    result = {
        "metric": METRIC.replace("DAF VGG16", f"{a.method.upper()} {'VGG16' if a.net == 'vgg16' else 'ResNet101'}"),
        "value": round(value, 4), "unit": "img/s", "n_gpus": world,
        "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(ms_per_step, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": f"{a.method.upper()} {a.net} "
                               f"{'PASCAL->Clipart' if ncls == 21 else 'Cityscapes->Foggy'} training step "
                               f"(methods/{a.method.upper()}/{a.method.upper()}_train.py), "
                               "1 source + 1 target image per GPU per step",
                   "image_hw": [a.height, a.width], "source_images_per_step": world,
                   "images_processed_per_step": 2 * world, "parallelism": f"dp{world}",
                   "classes": ncls, "rpn_pre_post_nms_train": [12000, 2000],
                   "rpn_pre_post_nms_test": [6000, 300],
                   "rcnn_batch": 256 if a.net == "vgg16" else 128},
        "roofline": roofline_entry(a, records, n_prof) if a.full else None,
        "conv_math": {"3x3 fwd/dgrad": tconv.conv_math(), "3x3 and 1x1 wgrad": tconv.wgrad_math(),
                      "1x1 fwd/dgrad": f"{tconv.conv_math()} (>= 64 channels on one side, "
                                       ">= 16 on the other; f32 MFMA for the 2-output DA "
                                       "image head)",
                      "fc6/fc7/DA fc": linear_math()},
        "rank_ms_per_step": {"min": round(min(per_rank) / a.steps * 1e3, 3),
                             "max": round(max(per_rank) / a.steps * 1e3, 3),
                             "spread_pct": round((max(per_rank) / min(per_rank) - 1) * 100, 2)},
        "mean_loss": round(last_loss, 4),
        # ReLU backward passes folded into the next conv's dgrad epilogue, per step (tlod.conv)
        "fused_relu_backward_per_step": {k: (v - stats0.get(k, 0)) / a.steps
                                         for k, v in tconv.STATS.items()},
        "cpu_baseline": None,
    }
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, model, losses)
    if a.full and rank == 0 and world == 1 and a.cpu_baseline_steps > 0 and a.method == "daf" \
            and a.net == "vgg16":
        result["cpu_baseline"] = cpu_baseline(a.cpu_baseline_steps, a.height, a.width,
                                              a.cpu_threads)
    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
