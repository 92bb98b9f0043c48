"""MXFP4-weight linear (ext.mxfp4_linear, csrc/mxfp4_linear.hip) against the
16-bit path (ops.linear.tuned_linear) and the one-launch fp8 kernel
(ext.fp8_linear_wide) on the Llama-2-7B / Llama-3-8B projection and LM-head
shapes at decode-sized batches (M <= 64).

  python benchmarks/mxfp4_linear_bench.py [--shapes 4096x4096,...] [--m 1,16]
      [--instances auto,4x4] [--swiglu] [--out table.md]

Per (N, K, M) all paths run alternating in one process; the comparison path
("fp8": ext.fp8_linear_wide, with --swiglu ext.fp8_swiglu_linear) runs first
and last, and the difference of its two windows is the run-to-run spread: a
ratio inside it counts as level. Each path cycles through enough weight copies
(>= 512 MiB of its own format) that no call finds its weights in a cache.
Times are device-event windows after a warm-up. "hbm%" is weight bytes / time
over the 8 TB/s HBM peak, on each format's own bytes: N*K for fp8, N*K/2 codes
plus N*K/32 scale bytes for MXFP4. --instances lists (waves x tiles) to force
on the MXFP4 kernel ("mx4/WxNT"; auto = its own choice). --swiglu times the
fused gate/up call instead: N is the intermediate size, bytes count both
weights, and the 16-bit column is left out.

Batch sizes above 64 (the tiled kernel ext.mxfp4_gemm) take other columns, in
one process as well: "w16" (tuned_linear on resident 16-bit weights) runs first
and last and carries the spread; "deq" is the path ops.mxfp4_linear took there
before mxfp4_gemm existed (ext.mxfp4_dequantize + tuned_linear); "fp8g" is
ext.fp8_gemm; "mx4g" is ext.mxfp4_gemm with its automatic K split (--splits
forces it, "mx4g/sN"). "mfma%" is 2*M*N*K / time over MFMA_PEAK. With --swiglu
the first-and-last column is "seq", the composition ops.mxfp4_swiglu_linear ran
there before (two deq + tuned_linear calls and swiglu), against "fused",
ext.mxfp4_swiglu_gemm; its FLOPs count both weights.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch  # noqa: E402

HBM_PEAK = 8.0e12   # bytes/s, MI355X
MFMA_PEAK = 2.5e15  # dense bf16 FLOP/s, MI355X
SHAPES = [(4096, 4096), (11008, 4096), (4096, 11008), (32000, 4096),
          (1024, 4096), (14336, 4096), (4096, 14336), (128256, 4096)]
MS = [1, 8, 16, 32, 64]


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
    p.add_argument("--instances", default="auto", metavar="WxNT,...")
    p.add_argument("--swiglu", action="store_true")
    p.add_argument("--splits", default="0",
                   help="M > 64: K splits to force on the tiled kernel, comma "
                        "separated (0 = automatic)")
    p.add_argument("--window-ms", type=float, default=40.0)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--out", default=None, help="also write a markdown table")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mxfp4_linear_bench needs a GPU: nothing is measured without")
    from torchacc_amd.ops import (quantize_weight_fp8, quantize_weight_mxfp4,
                                  swiglu)
    from torchacc_amd.ops._backend import require_extension
    from torchacc_amd.ops.linear import tuned_linear
    ext = require_extension()
    shapes = SHAPES if args.shapes is None else [
        tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    ms = MS if args.m is None else [int(v) for v in args.m.split(",")]
    inst = [(0, 0) if v == "auto" else tuple(int(c) for c in v.split("x"))
            for v in args.instances.split(",")]
    splits = [int(v) for v in args.splits.split(",")]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    pair = 2 if args.swiglu else 1
    rows = []
    torch.manual_seed(0)
    for n, k in shapes:
        # every format gets >= 512 MiB of copies of its own; --swiglu: copy i
        # is the gate weight, copy c + i the up weight
        c4 = max(2, -(-(512 << 20) // (n * k // 2)))
        c8 = max(2, -(-(512 << 20) // (n * k)))
        q4, q8, w16 = [], [], []
        for i in range(pair * c4):
            w = torch.randn(n, k, device="cuda", dtype=torch.bfloat16) * 0.02
            q4.append(quantize_weight_mxfp4(w))
            if i < pair * c8:
                q8.append(quantize_weight_fp8(w))
            if i < c8 and not args.swiglu:
                w16.append(w)
            del w
        for m in ms:
            x = torch.randn(m, k, device="cuda", dtype=torch.bfloat16)
            fns, cyc = {}, {}
            # the column run first and last
            base = "fp8" if m <= 64 else ("seq" if args.swiglu else "w16")

            def deq(i):     # the 16-bit transient of the path before mxfp4_gemm
                return ext.mxfp4_dequantize(*q4[i], x.dtype)

            if m > 64 and args.swiglu:
                fns["seq"] = lambda i: swiglu(tuned_linear(x, deq(i)),
                                              tuned_linear(x, deq(c4 + i)))
                cyc["seq"] = c4
                for sp in splits:
                    name = "fused" if sp == 0 else f"fused/s{sp}"
                    fns[name] = lambda i, sp=sp: ext.mxfp4_swiglu_gemm(
                        x, *q4[i], *q4[c4 + i], None, None, sp)
                    cyc[name] = c4
            elif m > 64:
                fns["w16"] = lambda i: tuned_linear(x, w16[i])
                fns["deq"] = lambda i: tuned_linear(x, deq(i))
                fns["fp8g"] = lambda i: ext.fp8_gemm(x, *q8[i])
                cyc.update(w16=c8, deq=c4, fp8g=c8)
                for sp in splits:
                    name = "mx4g" if sp == 0 else f"mx4g/s{sp}"
                    fns[name] = lambda i, sp=sp: ext.mxfp4_gemm(
                        x, *q4[i], None, sp)
                    cyc[name] = c4
            elif args.swiglu:
                fns["fp8"] = lambda i: ext.fp8_swiglu_linear(
                    x, *q8[i], *q8[c8 + i])
            else:
                fns["fp8"] = lambda i: ext.fp8_linear_wide(x, *q8[i])
                fns["w16"] = lambda i: tuned_linear(x, w16[i])
                cyc["w16"] = c8
            cyc["fp8"] = c8
            for wv, nt in inst if m <= 64 else []:
                name = "mx4" if wv == 0 else f"mx4/{wv}x{nt}"
                if args.swiglu:
                    fns[name] = lambda i, wv=wv, nt=nt: \
                        ext.mxfp4_swiglu_linear(x, *q4[i], *q4[c4 + i], None,
                                                None, wv, nt)
                else:
                    fns[name] = lambda i, wv=wv, nt=nt: ext.mxfp4_linear(
                        x, *q4[i], None, wv, nt)
                cyc[name] = c4
            fns[base + "b"], cyc[base + "b"] = fns[base], cyc[base]
            with torch.no_grad():
                est = {}
                for name, fn in fns.items():       # warm-up, sizes the window
                    _window(fn, cyc[name], cyc[name])
                    est[name] = _window(fn, cyc[name], 2 * cyc[name])
                t = {name: [] for name in fns}
                for _ in range(args.reps):
                    for name, fn in fns.items():
                        iters = max(20, int(args.window_ms * 1e3 / est[name]))
                        t[name].append(_window(fn, cyc[name], iters))
            us = {name: statistics.median(v) for name, v in t.items()}
            row = {"n": n, "k": k, "m": m, "swiglu": args.swiglu, "us": us,
                   "spread": abs(us[base] - us[base + "b"]) / us[base]}
            if m > 64:
                row["splits_auto"] = ext.mxfp4_gemm_num_splits(m, n, k, cus)
                old = "seq" if args.swiglu else "deq"
                for name in us:
                    if name.startswith(("mx4g", "fused", "fp8g")):
                        row[f"mfma_{name}"] = (2.0 * pair * m * n * k
                                               / (us[name] * 1e-6) / MFMA_PEAK)
                    if name.startswith(("mx4g", "fused")):
                        row[f"vs_{old}_{name}"] = us[name] / (
                            min(us["seq"], us["seqb"]) if args.swiglu
                            else us["deq"])
                rows.append(row)
                print(json.dumps(row), flush=True)
                continue
            row["instance"] = ext.mxfp4_linear_instance(n, k, cus, args.swiglu)
            for name in us:
                if name.startswith("fp8"):
                    nbytes = pair * n * k
                elif name.startswith("mx4"):
                    nbytes = pair * (n * k // 2 + n * k // 32)
                    row[f"ratio_{name}"] = us[name] / min(us["fp8"],
                                                          us["fp8b"])
                else:
                    continue
                row[f"hbm_{name}"] = nbytes / (us[name] * 1e-6) / HBM_PEAK
            rows.append(row)
            print(json.dumps(row), flush=True)
        del q4, q8, w16
    big = [r for r in rows if r["m"] > 64]
    rows = [r for r in rows if r["m"] <= 64]
    if args.out and big:
        base = "seq" if args.swiglu else "w16"
        names = [nm for nm in big[0]["us"] if nm not in (base, base + "b")]
        with open(args.out + (".gemm" if rows else ""), "w") as f:
            head = [f"{base} us", f"{base} again us", "spread", "S"]
            for nm in names:
                head.append(f"{nm} us")
                if nm != "deq":
                    head.append("mfma%")
                if nm.startswith(("mx4g", "fused")):
                    head.append("vs " + ("seq" if args.swiglu else "deq"))
            f.write("| N | K | M | " + " | ".join(head) + " |\n")
            f.write("|" + "---|" * (3 + len(head)) + "\n")
            for r in big:
                us = r["us"]
                cells = [r["n"], r["k"], r["m"], f"{us[base]:.1f}",
                         f"{us[base + 'b']:.1f}", f"{r['spread']:.1%}",
                         r["splits_auto"]]
                for nm in names:
                    cells.append(f"{us[nm]:.1f}")
                    if nm != "deq":
                        cells.append(f"{r['mfma_' + nm]:.1%}")
                    if nm.startswith(("mx4g", "fused")):
                        key = "vs_seq_" if args.swiglu else "vs_deq_"
                        cells.append(f"{r[key + nm]:.2f}")
                f.write("| " + " | ".join(str(c) for c in cells) + " |\n")
    if args.out and rows:
        names = [nm for nm in rows[0]["us"] if nm.startswith("mx4")]
        with open(args.out, "w") as f:
            head = [] if args.swiglu else ["16-bit us"]
            head += ["fp8 us", "hbm%", "fp8 again us", "spread", "W x NT"]
            for nm in names:
                head += [f"{nm} us", "hbm%", "vs fp8"]
            f.write("| N | K | M | " + " | ".join(head) + " |\n")
            f.write("|" + "---|" * (3 + len(head)) + "\n")
            for r in rows:
                us = r["us"]
                cells = [r["n"], r["k"], r["m"]]
                if not args.swiglu:
                    cells.append(f"{us['w16']:.1f}")
                cells += [f"{us['fp8']:.1f}", f"{r['hbm_fp8']:.0%}",
                          f"{us['fp8b']:.1f}", f"{r['spread']:.1%}",
                          "{}x{}".format(*r["instance"])]
                for nm in names:
                    cells += [f"{us[nm]:.1f}", f"{r['hbm_' + nm]:.0%}",
                              f"{r['ratio_' + nm]:.2f}"]
                f.write("| " + " | ".join(str(c) for c in cells) + " |\n")


if __name__ == "__main__":
    main()
