#!/usr/bin/env python3
"""One decode / chunk step on a persistent KV cache -- ``cache.append`` of T rows, then ``sageattn_splitkv_cached`` -- against
the uncached ``sageattn_splitkv`` / ``sageattn_splitkv_causal`` call on the same tensors, measured as tools/splitkv_bench.py
measures: ONE process, the variants of a comparison timed round robin in `--repeats` rounds, each window 3 warm-up calls and
HIP events around about `--window-ms` of calls; a time is the median over the rounds, a ratio the median of the per-round
ratios with its least and greatest value.  The uncached call is the yardstick and is timed twice per rotation ("uncached
again"): its spread against itself is what a gain has to leave behind.

  (8, 32, 1, 8192, 128) folded by the GQA group 4: q [8, 8, 4, 128]      a decode step, T = 1
  (1, 32, 128, 65536, 128)                                               a speculative chunk over a long cache, T = 128
  (1, 40, 512, 32760, 128)                                               text / latent queries over a video context, T = 512
  causal (8, 8, 16, 8192, 128), q_fold = 4                               4 speculative tokens, T = 4

Every batch holds N keys (kv_lens = N on the device); the step appends the rows [N - T, N) each time -- the work of a real
step, on lengths that do not move, so that every timed call is the same call.  Kernel times: mean device time from a
torch.profiler trace of 5 steps.  Also: what ``SageKVCache.prepare`` costs against one uncached call.  Acceptance: at every
shape the cached step's slowest round relative to the yardstick lies below the fastest "uncached again" round; where it does
not, the table says NO.

``--drift-log FILE``: lines ``KVCACHE_DRIFT ...`` printed by tests/test_kvcache_gpu.py (pytest -s) become the drift table;
``--append FILE``: a text file (the alternating ``bench.py`` rounds) is appended as it is.

usage: kvcache_bench.py [--repeats 5] [--window-ms 100] [--pv fp16,fp8] [--commit HASH] [--drift-log F] [--append F]
                        [--out profiles/kv_cache.md]"""
import argparse
import os
import re
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import sageattention_amd as sa  # noqa: E402
from sageattention_amd import core  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--window-ms", type=float, default=100.0)
ap.add_argument("--pv", default="fp16,fp8")
ap.add_argument("--commit", default="")
ap.add_argument("--drift-log", default="")
ap.add_argument("--append", default="")
ap.add_argument("--out", default="")
a = ap.parse_args()
lines = []


def emit(s=""):
    print(s, flush=True)
    lines.append(s)


def events(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n  # ms per call


def rounds(variants):
    """variants: name -> callable.  Round robin, a.repeats rounds -> name -> [ms per call of every round]"""
    calls = {}
    for name, fn in variants.items():  # first launches load code objects; then size the window of this variant
        for _ in range(3):
            fn()
        calls[name] = max(5, int(a.window_ms / max(events(fn, 3), 1e-3)))
    out = {name: [] for name in variants}
    for _ in range(a.repeats):
        for name, fn in variants.items():
            for _ in range(3):
                fn()
            out[name].append(events(fn, calls[name]))
    return out


def med(ts):
    return statistics.median(ts)


def ratios(ts, base):
    return [x / y for x, y in zip(ts, base)]


def fmt_ratio(r):
    return f"{med(r):.3f} ({min(r):.3f} .. {max(r):.3f})"


def kernel_times(fn, names, calls=5):
    """mean device time (us) per call of the kernels whose names contain each of ``names`` -> {name: us}, {} without a trace"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        out = {}
        for it in prof.key_averages():
            tot = 0.0
            for attr in ("self_device_time_total", "device_time_total", "self_cuda_time_total", "cuda_time_total"):
                tot = getattr(it, attr, 0.0) or 0.0
                if tot:
                    break
            for n in names:
                if tot and n in it.key:
                    out[n] = out.get(n, 0.0) + tot / calls
                    break
        return out
    except Exception as exc:  # the trace is a listing beside the timed calls, not one of them
        print(f"(no kernel trace: {exc})", flush=True)
        return {}


def make(B, Hq, Hk, M, N, D, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = torch.randn(B, Hq, M, D, generator=g, device="cuda").half()
    k = (torch.randn(B, Hk, N, D, generator=g, device="cuda") + 0.5 * torch.randn(B, Hk, 1, D, generator=g, device="cuda")).half()
    v = torch.randn(B, Hk, N, D, generator=g, device="cuda").half()
    return q, k, v


if not torch.cuda.is_available():
    sys.exit("kvcache_bench.py measures on the GPU: none is visible")

# (label, (B, Hq, Hk, M, N, D) as the operator sees it, T rows appended per step, q_fold or None: non-causal)
SHAPES = [("(8, 32, 1, 8192, 128) folded by the GQA group 4: q [8, 8, 4, 128], T = 1", (8, 8, 8, 4, 8192, 128), 1, None),
          ("(1, 32, 128, 65536, 128), T = 128", (1, 32, 32, 128, 65536, 128), 128, None),
          ("(1, 40, 512, 32760, 128), T = 512", (1, 40, 40, 512, 32760, 128), 512, None),
          ("causal (8, 8, 16, 8192, 128), q_fold = 4, T = 4", (8, 8, 8, 16, 8192, 128), 4, 4)]
PRE = ("k_mean_partial", "kv_partial", "k_quant_stream", "kv_quant")   # the uncached call's pre-pass kernels
KERNELS = ("kv_cache_append_kernel", "attn_i8_splitkv", "splitkv_merge_kernel") + PRE

emit("# A persistent quantized KV cache for the split-KV operators: step times on MI355X")
emit()
emit(f"commit {a.commit or 'unknown'}; tools/kvcache_bench.py, one process, the variants of a comparison timed round robin in")
emit(f"{a.repeats} rounds, a window = 3 warm-up calls and HIP events around about {a.window_ms:.0f} ms of calls.  fp16 inputs, per-thread")
emit("scales, kv_lens = N for every batch (on the device), the automatic split count.  \"uncached\": the whole sageattn_splitkv /")
emit("sageattn_splitkv_causal call (length-aware pre-pass + attention + merge).  \"cached step\": cache.append of the last T rows +")
emit("sageattn_splitkv_cached (one append launch + attention + merge).  Times: median over the rounds.  Ratios: median of the")
emit("per-round ratios (least .. greatest) to \"uncached\"; \"uncached again\" is the yardstick timed a second time in the same")
emit("rotation.  Kernel columns: mean device time per step from a torch.profiler trace of 5 steps (pre-pass: its kernels summed).")
verdicts, prepares = [], []
for label, (B, Hq, Hk, M, N, D), T, fold in SHAPES:
    S = core.splitkv_num_splits(B, Hq, M, N)
    emit()
    emit(f"## {label}")
    emit()
    emit(f"S = {S} (the automatic choice)")
    emit()
    emit("| PV | variant | ms | / uncached | pre-pass us | append us | attention us | merge us |")
    emit("|---|---|---|---|---|---|---|---|")
    q, k, v = make(B, Hq, Hk, M, N, D, 1)
    lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
    start = torch.full((B,), N - T, dtype=torch.int32, device="cuda")
    for pv in a.pv.split(","):
        cache = sa.SageKVCache.prepare(k, v, lens, pv=pv)
        if fold is None:
            uncached = lambda: sa.sageattn_splitkv(q, k, v, lens, S, pv=pv)  # noqa: E731
        else:
            uncached = lambda: sa.sageattn_splitkv_causal(q, k, v, lens, S, fold, pv=pv)  # noqa: E731

        def step():
            cache.append(start, lens, T)
            return sa.sageattn_splitkv_cached(q, cache, lens, S, causal=fold is not None, q_fold=fold or 1)

        torch.cuda.synchronize()
        variants = {"uncached": uncached, "uncached again": uncached, "cached step": step,
                    "prepare": lambda: sa.SageKVCache.prepare(k, v, lens, pv=pv)}
        t = rounds(variants)
        again = ratios(t["uncached again"], t["uncached"])
        for name in variants:
            kt = kernel_times(variants[name], KERNELS) if name in ("uncached", "cached step") else {}
            pre = sum(kt.get(n, 0.0) for n in PRE)
            cols = [f"{pre:.1f}" if pre else "", *(f"{kt[n]:.1f}" if n in kt else "" for n in KERNELS[:3])]
            r = "" if name == "uncached" else fmt_ratio(ratios(t[name], t["uncached"]))
            emit(f"| {pv} | {name} | {med(t[name]):.4f} | {r} | " + " | ".join(cols) + " |")
        rs = ratios(t["cached step"], t["uncached"])
        verdicts.append((label, pv, med(rs), max(rs), min(again), max(again), max(rs) < min(again) and max(rs) < 1.0))
        prepares.append((label, pv, med(t["prepare"]), med(ratios(t["prepare"], t["uncached"]))))
        del cache
    del q, k, v
    torch.cuda.empty_cache()

emit()
emit("## Cached step against the uncached call")
emit()
emit("Acceptance: the cached step's slowest round relative to the yardstick lies below the fastest \"uncached again\" round.")
emit()
emit("| shape | PV | cached step / uncached (median, greatest) | uncached again / uncached (least .. greatest) | met |")
emit("|---|---|---|---|---|")
for label, pv, m, mx, lo, hi, ok in verdicts:
    emit(f"| {label} | {pv} | {m:.3f}, {mx:.3f} | {lo:.3f} .. {hi:.3f} | {'yes' if ok else 'NO'} |")
emit()
emit("## What prepare costs")
emit()
emit("SageKVCache.prepare: the length-aware pre-pass, and for FP8 P.V the frozen V scale (a few small torch kernels) and the V^T")
emit("image written again under it (one append launch over all tiles); paid once per cache, or per re-prepared slot.")
emit()
emit("| shape | PV | prepare ms | / one uncached call |")
emit("|---|---|---|---|")
for label, pv, ms, r in prepares:
    emit(f"| {label} | {pv} | {ms:.4f} | {r:.2f} |")

if a.drift_log and os.path.exists(a.drift_log):
    rows = re.findall(r"KVCACHE_DRIFT D=(\d+) pv=(\w+) ([\w-]+): cached o (\S+) lse (\S+) \| uncached o (\S+) lse (\S+) \| ratio o (\S+) "
                      r"lse (\S+)", open(a.drift_log).read())
    emit()
    emit("## Frozen statistics on data that drifts")
    emit()
    emit("tests/test_kvcache_gpu.py::test_frozen_statistics_on_drifting_data: N = 1000, (2, 4 on 2, 70 rows), the cache prepared at")
    emit("250 keys and grown to 1000; max abs error against float64 attention on the same fp16 inputs, beside the uncached")
    emit("sageattn_splitkv on all 1000 keys.  The test admits a ratio of at most 2.  v-drift: the V rows from 250 on reach 1.5x the")
    emit("prefix maximum (headroom 2.0: nothing saturates).")
    emit()
    emit("| D | PV | data | cached o | cached lse | uncached o | uncached lse | ratio o | ratio lse |")
    emit("|---|---|---|---|---|---|---|---|---|")
    for row in rows:
        emit("| " + " | ".join(row) + " |")
if a.append and os.path.exists(a.append):
    emit()
    emit(open(a.append).read().rstrip())
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
