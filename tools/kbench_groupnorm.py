#!/usr/bin/env python3
"""GroupNorm against the InstanceNorm kernels at equal (B, HW, C), fp32 tokens, forward and backward, alternating in one process.
Times come from a kernel trace, not from this script:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/kbench_groupnorm.py
  python tools/kbench_groupnorm.py --summarise OUT > profiles/groupnorm_vs_instnorm.txt

The run is ROUNDS + 1 rounds per shape (the first is warm-up and dropped) of REPS instnorm fwd+bwd then REPS groupnorm fwd+bwd; the
summary splits each kernel's dispatches, in order, back into (shape, round), takes the mean per round, and reports the median over
rounds and the spread (max - min over rounds, relative to the median).  A pass = its two kernels (stats + apply); the second-stage
folds of the parameter gradients (one launch for instnorm, two for groupnorm; queued and batched inside a training step) are not part of it."""
import csv, glob, os, re, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "adnm-unet_amd"))

SHAPES = [(4, 16384, 32, 4), (4, 16384, 64, 8), (4, 4096, 128, 4)]
ROUNDS, REPS = 5, 40
KERNELS = ["stats", "apply", "bwd_stats", "bwd_apply"]
BYTES = {"stats": 1, "apply": 2, "bwd_stats": 2, "bwd_apply": 3}   # tensor passes: fwd reads x twice + writes y; bwd reads dy, x twice + writes dx
PEAK = 8.0e12   # HBM3E spec peak, bytes / s


def run():
    import torch
    from adnm_hip import ops, lib
    dev = "cuda"
    for B, HW, C, G in SHAPES:
        x, dy = torch.randn(B, HW, C, device=dev) * 2 + 1, torch.randn(B, HW, C, device=dev)
        w, b = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
        sc, sh = torch.tensor(0.9, device=dev), torch.tensor(0.15, device=dev)
        for _ in range(ROUNDS + 1):
            for _ in range(REPS):
                y, mu, rstd = ops.k_instnorm_fwd(x, sc, sh, B, HW, C, 1e-5, lib.ACT_GELU)
                ops.k_instnorm_bwd(dy, x, sc, sh, mu, rstd, B, HW, C, lib.ACT_GELU)
            for _ in range(REPS):
                y, mu, rstd = ops.k_groupnorm_fwd(x, G, w, b, sc, sh, B, HW, C, 1e-5, lib.ACT_GELU)
                ops.k_groupnorm_bwd(dy, x, G, w, b, sc, sh, mu, rstd, B, HW, C, lib.ACT_GELU)
            torch.cuda.synchronize()


def summarise(out_dir):
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"expected one *kernel_trace.csv under {out_dir}, found {files}")
    pat = re.compile(r"(instnorm|groupnorm)_(bwd_stats|bwd_apply|stats|apply)_kernel")
    per = {}
    with open(files[0]) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        m = pat.search(r["Kernel_Name"])
        if m:
            per.setdefault((m.group(1), m.group(2)), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    n = len(SHAPES) * (ROUNDS + 1) * REPS
    for k, v in per.items():
        if len(v) != n:
            raise SystemExit(f"{k}: {len(v)} dispatches in the trace, expected {n}")

    def cell(norm, kern, si):   # -> (median over rounds of the per-round mean, spread)
        v = per[(norm, kern)]
        means = [statistics.mean(v[(si * (ROUNDS + 1) + rd) * REPS:(si * (ROUNDS + 1) + rd + 1) * REPS]) for rd in range(1, ROUNDS + 1)]
        med = statistics.median(means)
        return med, (max(means) - min(means)) / med, means

    print(f"# fp32 tokens, act GELU, {ROUNDS} rounds x {REPS} launches per kernel and shape, alternating instnorm / groupnorm in one process; us per launch")
    print("# (B,HW,C,G)          kernel      instnorm  spread   groupnorm  spread   ratio   groupnorm GB/s  of 8 TB/s")
    for si, (B, HW, C, G) in enumerate(SHAPES):
        tot = {"fwd": [0.0, 0.0, None, None], "bwd": [0.0, 0.0, None, None]}
        for kern in KERNELS:
            (ti, si_, mi), (tg, sg, mg) = cell("instnorm", kern, si), cell("groupnorm", kern, si)
            by = 4.0 * B * HW * C * BYTES[kern]
            print(f"({B},{HW},{C},{G})".ljust(22) + f"{kern:<11} {ti:8.2f}  {100 * si_:5.1f}%  {tg:9.2f}  {100 * sg:5.1f}%  {tg / ti:6.3f}  {by / tg / 1e3:12.0f}  {by / (tg * 1e-6) / PEAK:9.3f}")
            p = tot["bwd" if kern.startswith("bwd") else "fwd"]
            p[2] = mi if p[2] is None else [a + b for a, b in zip(p[2], mi)]
            p[3] = mg if p[3] is None else [a + b for a, b in zip(p[3], mg)]
        for name, (_, _, mi, mg) in tot.items():
            ti, tg = statistics.median(mi), statistics.median(mg)
            si_, sg = (max(mi) - min(mi)) / ti, (max(mg) - min(mg)) / tg
            by = 4.0 * B * HW * C * (3 if name == "fwd" else 5)
            print(f"({B},{HW},{C},{G})".ljust(22) + f"{name + ' pass':<11} {ti:8.2f}  {100 * si_:5.1f}%  {tg:9.2f}  {100 * sg:5.1f}%  {tg / ti:6.3f}  {by / tg / 1e3:12.0f}  {by / (tg * 1e-6) / PEAK:9.3f}")


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2])
    else:
        run()
