"""fp8-weight linear (ops.fp8_linear, csrc/fp8_linear.hip) against the 16-bit
path (ops.linear.tuned_linear) on the Llama-2-7B / Llama-3-8B projection and
LM-head shapes, decode-sized batches (the skinny kernel) and prefill-sized
ones (the tiled fp8_gemm kernel).

  python benchmarks/fp8_linear_bench.py [--shapes 4096x4096,...] [--m 1,16]
      [--splits 0,1,4] [--out table.md]

Per (N, K, M) the two paths run alternating in one process, 16-bit first and
last, so the difference of the two 16-bit windows shows the run-to-run
spread. Each path cycles through enough weight copies (>= 512 MiB) that no
call finds its weights in a cache. Times are device-event windows after a
warm-up. "hbm%" is weight bytes / time over the 8 TB/s HBM peak. --splits
lists K-split counts to force on the kernel (0 = its own choice). The fp8
column is the kernel itself at every M, also above FP8_LINEAR_MAX_M where
ops.fp8_linear would not route to it: that is how the crossover is found.

Above M = 64 two more columns run in the same alternation: "deq", the path
ops.fp8_linear took there before fp8_gemm existed, written out here
(dequantise the weight in memory, then tuned_linear), and "gemm", the tiled
kernel ext.fp8_gemm (--splits also forces its K split, "gemm/sN"). For the
gemm columns "mfma%" is 2*M*N*K / time over MFMA_PEAK.

--one-launch adds, through M = 64, the one-launch kernel ext.fp8_linear_wide
("one", or "one/WxNT" for a forced instance). --swiglu times the MLP
up-projection instead: "seq" = two ops.fp8_linear calls and ops.swiglu, run
first and last as the comparison, against "fused" = ext.fp8_swiglu_linear
("fused/W" for forced waves); N is then the intermediate size and hbm% counts
both weights.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch  # noqa: E402

HBM_PEAK = 8.0e12   # bytes/s, MI355X
# dense bf16/fp16 matrix peak of the MI355X, FLOP/s: AMD's product
# specification (2.5 PFLOP/s without sparsity)
MFMA_PEAK = 2.5e15
SHAPES = [(4096, 4096), (11008, 4096), (4096, 11008), (32000, 4096),
          (1024, 4096), (14336, 4096), (4096, 14336), (128256, 4096)]
MS = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096]
SKINNY_MAX_M = 128   # the skinny kernel is timed up to here


def _window(fn, copies, iters):
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    start.record()
    for i in range(iters):
        fn(i % copies)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters * 1e3   # us per call


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", default=None, help="NxK,NxK,...")
    p.add_argument("--m", default=None, help="batch sizes, comma separated")
    p.add_argument("--splits", default="0")
    p.add_argument("--one-launch", default=None, metavar="WxNT,...",
                   help="also time the one-launch kernel (M <= 64): 'auto' "
                        "or forced instances such as 4x2,8x1 ('one/WxNT')")
    p.add_argument("--swiglu", action="store_true",
                   help="time the fused gate/up call ('fused', M <= 64) "
                        "against gate + up + swiglu on ops.fp8_linear "
                        "('seq') instead of the single projection; "
                        "--one-launch then lists waves only (auto,4,8)")
    p.add_argument("--window-ms", type=float, default=40.0)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--out", default=None, help="also write a markdown table")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fp8_linear_bench needs a GPU: nothing is measured without")
    from torchacc_amd.ops import fp8_linear, quantize_weight_fp8, swiglu
    from torchacc_amd.ops._backend import require_extension
    from torchacc_amd.ops.linear import tuned_linear
    ext = require_extension()
    shapes = SHAPES if args.shapes is None else [
        tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    ms = MS if args.m is None else [int(v) for v in args.m.split(",")]
    splits = [int(v) for v in args.splits.split(",")]
    # forced (waves, tiles) of the one-launch kernel; (0, 0) = its own choice
    wide = [] if args.one_launch is None else [
        (0, 0) if v == "auto"
        else tuple(int(c) for c in (v + "x0").split("x")[:2])
        for v in args.one_launch.split(",")]
    base = "seq" if args.swiglu else "w16"   # the column run first and last
    rows = []
    torch.manual_seed(0)
    for n, k in shapes:
        copies = max(2, -(-(512 << 20) // (n * k)))
        # --swiglu: copy i is the gate weight, copy copies + i the up weight
        w16 = [torch.randn(n, k, device="cuda", dtype=torch.bfloat16) * 0.02
               for _ in range(2 * copies if args.swiglu else copies)]
        q = [quantize_weight_fp8(w) for w in w16]
        for m in ms:
            x = torch.randn(m, k, device="cuda", dtype=torch.bfloat16)
            if args.swiglu:
                fns = {"seq": lambda i: swiglu(
                    fp8_linear(x, *q[i]), fp8_linear(x, *q[copies + i]))}
                for wv, _ in wide if m <= 64 else []:
                    name = "fused" if wv == 0 else f"fused/{wv}"
                    fns[name] = lambda i, wv=wv: ext.fp8_swiglu_linear(
                        x, *q[i], *q[copies + i], None, None, wv)
            else:
                fns = {"w16": lambda i: tuned_linear(x, w16[i])}
            for s in splits if m <= SKINNY_MAX_M and not args.swiglu else []:
                name = "fp8" if s == 0 else f"fp8/s{s}"
                fns[name] = lambda i, s=s: ext.fp8_linear(
                    x, q[i][0], q[i][1], None, s)
            for wv, nt in wide if m <= 64 and not args.swiglu else []:
                name = "one" if wv == 0 else f"one/{wv}x{nt}"
                fns[name] = lambda i, wv=wv, nt=nt: ext.fp8_linear_wide(
                    x, q[i][0], q[i][1], None, wv, nt)
            if m > 64 and not args.swiglu:
                fns["deq"] = lambda i: tuned_linear(
                    x, (q[i][0].float() * q[i][1][:, None]).to(x.dtype), None)
                for s in splits:
                    name = "gemm" if s == 0 else f"gemm/s{s}"
                    fns[name] = lambda i, s=s: ext.fp8_gemm(
                        x, q[i][0], q[i][1], None, s)
            fns[base + "b"] = fns[base]
            with torch.no_grad():
                est = {}
                for name, fn in fns.items():       # warm-up, sizes the window
                    _window(fn, copies, copies)
                    est[name] = _window(fn, copies, 2 * copies)
                t = {name: [] for name in fns}
                for _ in range(args.reps):
                    for name, fn in fns.items():
                        iters = max(20, int(args.window_ms * 1e3 / est[name]))
                        t[name].append(_window(fn, copies, iters))
            us = {name: statistics.median(v) for name, v in t.items()}
            cus = torch.cuda.get_device_properties(0).multi_processor_count
            row = {"n": n, "k": k, "m": m, "us": us,
                   "spread": abs(us[base] - us[base + "b"]) / us[base],
                   "splits_auto": ext.fp8_linear_num_splits(n, k, cus),
                   "gemm_splits_auto": ext.fp8_gemm_num_splits(m, n, k, cus)}
            for name in us:
                if name.startswith(("fp8", "one", "fused")):
                    row[f"hbm_{name}"] = ((2 if args.swiglu else 1) * n * k
                                          / (us[name] * 1e-6) / HBM_PEAK)
                if name.startswith("gemm"):
                    row[f"mfma_{name}"] = (2.0 * m * n * k
                                           / (us[name] * 1e-6) / MFMA_PEAK)
                    row[f"vs_deq_{name}"] = us[name] / us["deq"]
                if name not in (base, base + "b"):
                    row[f"ratio_{name}"] = us[name] / min(us[base],
                                                          us[base + "b"])
            rows.append(row)
            print(json.dumps(row), flush=True)
        del w16, q
    if args.out:
        label = "gate+up+swiglu" if args.swiglu else "16-bit"
        with open(args.out, "w") as f:
            # one table per column set: M <= 64 has no deq/gemm columns
            for names in sorted({tuple(nm for nm in r["us"]
                                       if nm not in (base, base + "b"))
                                 for r in rows}, key=len):
                head = []
                for nm in names:
                    head.append(f"{nm} us")
                    if nm.startswith(("fp8", "one", "fused")):
                        head.append("hbm%")
                    if nm.startswith("gemm"):
                        head += ["mfma%", "vs deq"]
                    head.append(f"vs {label}")
                f.write(f"| N | K | M | {label} us | {label} again us | "
                        "spread | " + " | ".join(head) + " |\n")
                f.write("|" + "---|" * (6 + len(head)) + "\n")
                for r in rows:
                    if tuple(nm for nm in r["us"]
                             if nm not in (base, base + "b")) != names:
                        continue
                    cells = [r["n"], r["k"], r["m"], f"{r['us'][base]:.1f}",
                             f"{r['us'][base + 'b']:.1f}", f"{r['spread']:.1%}"]
                    for nm in names:
                        cells.append(f"{r['us'][nm]:.1f}")
                        if nm.startswith(("fp8", "one", "fused")):
                            cells.append(f"{r['hbm_' + nm]:.0%}")
                        if nm.startswith("gemm"):
                            cells += [f"{r['mfma_' + nm]:.1%}",
                                      f"{r['vs_deq_' + nm]:.2f}"]
                        cells.append(f"{r['ratio_' + nm]:.2f}")
                    f.write("| " + " | ".join(str(c) for c in cells) + " |\n")
                f.write("\n")


if __name__ == "__main__":
    main()
