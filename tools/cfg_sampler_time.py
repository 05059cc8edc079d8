"""The class-conditional sampler batch WITH classifier-free guidance (MaskGIT.cfg_scale = 2):
bench.py's sampler-leg MaskGIT (config B, the bench's stage2 weights), one GraphedSampler batch
(10 LF + 1 HF decoding steps, LF/HF decoders) timed per replay with device events; the median
of the replays, as one JSON line.  bench.py's own sampler leg is the unguided figure.

usage: python tools/cfg_sampler_time.py [--num 1024] [--reps 40] [--warmup 5] [--unfused]
  --unfused   bidirectional_transformer.FUSED_SAMPLE = False: the two forwards' logits are
              written, mixed by torch and read back by tvq_maskgit_sample (the only guided path
              before the guided launches existed)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "t-vq-vae-trajgen_amd"))
import torch  # noqa: E402

import bench  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--num", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cfg-scale", type=float, default=2.0)
    ap.add_argument("--class-index", type=int, default=1)
    ap.add_argument("--unfused", action="store_true")
    args = ap.parse_args()
    if args.reps < 30:
        ap.error("--reps must be at least 30 (the figure is a median)")

    from timevqvae.hip._native import plan_trace
    from timevqvae.models import bidirectional_transformer as bt
    from timevqvae.utils.sample_utils import GraphedSampler
    dev = torch.device("cuda", 0)
    mg = bench.JointTrainer(dev, 1).s2.maskgit.eval()
    mg.cfg_scale = args.cfg_scale
    if args.unfused:
        bt.FUSED_SAMPLE = False
    with torch.no_grad(), plan_trace() as tr:  # which launches a batch takes
        mg.iterative_decoding(num=args.num, device=dev, class_index=args.class_index)
        torch.cuda.synchronize()
    guided = sum(1 for s in tr.lines if s.startswith(("prior_lf_eval_sample_cfg",
                                                       "tied_logits_sample_cfg")))
    gs = GraphedSampler(mg, args.num, dev, class_index=args.class_index)
    for _ in range(args.warmup):
        gs.sample()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        gs.sample()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    ms.sort()
    print(json.dumps({"tool": "cfg_sampler_time", "num": args.num, "cfg_scale": args.cfg_scale,
                      "class_index": args.class_index, "unfused": bool(args.unfused),
                      "guided_fused_launches_per_batch": guided,
                      "ms_per_batch_median": round(statistics.median(ms), 4),
                      "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
                      "reps": args.reps, "warmup": args.warmup,
                      "trajectories_per_s": round(args.num / statistics.median(ms) * 1e3, 1)}),
          flush=True)
