#!/usr/bin/env python3
"""One decode / chunk step on the PAGED MXFP4 V cache -- ``SagePagedKVCacheV4.append`` of T rows, then
``sageattn_splitkv_paged_v4`` -- against two yardsticks, measured as tools/paged_bench.py measures: ONE process, the variants
of a comparison timed round robin in `--repeats` rounds, each window 3 warm-up calls and HIP events around about `--window-ms`
of calls; a time is the median over the rounds, a ratio the median of the per-round ratios with its least and greatest value.

  1. the contiguous ``SageKVCacheV4`` step on the padded tensors gathered from the pages: what paging costs.  It is timed twice
     per rotation ("contiguous fp4 again"): its spread against itself is what a difference has to leave behind.
  2. the ``SagePagedKVCache(pv="fp8")`` step on the same pools: the number a user chooses by.

  (8, 32, 1, 8192, 128) folded by the GQA group 4: q [8, 8, 4, 128]      a decode step, T = 1
  causal (8, 8, 16, 8192, 128), q_fold = 4                               4 speculative tokens, T = 4
  (1, 40, 512, 32760, 128)                                               text / latent queries over a video context, T = 512

Page sizes 64 and 256, the table a random permutation of all pages.  Every batch holds N keys; the step appends the rows
[N - T, N) each time, so that every timed call is the same call.  Kernel times: mean device time from a torch.profiler trace
of 5 steps, taken after the timing.

usage: paged_fp4_bench.py [--repeats 5] [--window-ms 100] [--commit HASH] [--out FILE]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import sageattention_amd as sa  # noqa: E402
from sageattention_amd import core  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--window-ms", type=float, default=100.0)
ap.add_argument("--commit", default="")
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


def to_pages(x, page_size, table):
    """the padded [B,Hk,Ncap,D] tensor cut into pages: pool [P,Hk,page_size,D] with page table[b, i] = rows i * page_size .."""
    B, Hk, Ncap, D = x.shape
    mp = Ncap // page_size
    pool = torch.empty((B * mp, Hk, page_size, D), dtype=x.dtype, device=x.device)
    pool[table.reshape(-1).long()] = x.view(B, Hk, mp, page_size, D).permute(0, 2, 1, 3, 4).reshape(B * mp, Hk, page_size, D)
    return pool


if not torch.cuda.is_available():
    sys.exit("paged_fp4_bench.py measures on the GPU: none is visible")

# (label, (B, Hq, Hk, M, N, D) as the operator sees it, T rows appended per step, q_fold or None: non-causal)
SHAPES = [("(8, 32, 1, 8192, 128) folded by the GQA group 4: q [8, 8, 4, 128], T = 1", (8, 8, 8, 4, 8192, 128), 1, None),
          ("causal (8, 8, 16, 8192, 128), q_fold = 4, T = 4", (8, 8, 8, 16, 8192, 128), 4, 4),
          ("(1, 40, 512, 32760, 128), T = 512", (1, 40, 40, 512, 32760, 128), 512, None)]
KERNELS = ("kv_cache_append", "attn_i8_splitkv", "splitkv_merge_kernel")

emit("# A paged MXFP4 V cache for the split-KV operators: step times on MI355X")
emit()
emit(f"commit {a.commit or 'unknown'}; tools/paged_fp4_bench.py, one process, the variants of a comparison timed round robin in")
emit(f"{a.repeats} rounds, a window = 3 warm-up calls and HIP events around about {a.window_ms:.0f} ms of calls.  fp16 inputs, per-thread")
emit("scales, kv_lens = N for every batch (on the device), the automatic split count.  \"contiguous fp4\": SageKVCacheV4.append of the")
emit("last T rows + sageattn_splitkv_v4 on the padded tensors (capacity = N rounded up to 256 keys).  \"paged fp4\":")
emit("SagePagedKVCacheV4.append + sageattn_splitkv_paged_v4 on the same rows cut into pages of 64 or 256 keys, the table a random")
emit("permutation of all pages.  \"paged fp8\": SagePagedKVCache(pv=\"fp8\").append + sageattn_splitkv_paged on the same pools and")
emit("table.  Times: median over the rounds.  Ratios: median of the per-round ratios (least .. greatest); \"contiguous fp4 again\"")
emit("is the first yardstick timed a second time in the same rotation.  Kernel columns: mean device time per step from a")
emit("torch.profiler trace of 5 steps, run after the timing.")
verdicts = []
for label, (B, Hq, Hk, M, N, D), T, fold in SHAPES:
    Ncap = (N + 255) // 256 * 256
    S = core.splitkv_num_splits(B, Hq, M, Ncap)
    emit()
    emit(f"## {label}")
    emit()
    emit(f"S = {S} (the automatic choice), capacity {Ncap} keys")
    emit()
    emit("| variant | ms | / contiguous fp4 | / paged fp8 of its page size | append us | attention us | merge us |")
    emit("|---|---|---|---|---|---|---|")
    g = torch.Generator(device="cuda").manual_seed(1)
    q = torch.randn(B, Hq, M, D, generator=g, device="cuda").half()
    k = (torch.randn(B, Hk, Ncap, D, generator=g, device="cuda") + 0.5 * torch.randn(B, Hk, 1, D, generator=g, device="cuda")).half()
    v = torch.randn(B, Hk, Ncap, D, generator=g, device="cuda").half()
    lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
    start = torch.full((B,), N - T, dtype=torch.int32, device="cuda")
    kw = dict(causal=fold is not None, q_fold=fold or 1)
    ref = sa.SageKVCacheV4.prepare(k, v, lens)

    def contiguous():
        ref.append(start, lens, T)
        return sa.sageattn_splitkv_v4(q, ref, lens, S, **kw)

    variants = {"contiguous fp4": contiguous, "contiguous fp4 again": contiguous}
    keep = []
    for ps in (64, 256):
        mp = Ncap // ps
        table = torch.randperm(B * mp, generator=torch.Generator().manual_seed(ps)).to(torch.int32).view(B, mp).cuda()
        k_pool, v_pool = to_pages(k, ps, table), to_pages(v, ps, table)
        c4 = sa.SagePagedKVCacheV4.prepare(k_pool, v_pool, table, lens)
        c8 = sa.SagePagedKVCache.prepare(k_pool, v_pool, table, lens, pv="fp8")
        keep += [c4, c8]

        def step4(c4=c4, table=table):
            c4.append(table, start, lens, T)
            return sa.sageattn_splitkv_paged_v4(q, c4, table, lens, S, **kw)

        def step8(c8=c8, table=table):
            c8.append(table, start, lens, T)
            return sa.sageattn_splitkv_paged(q, c8, table, lens, S, **kw)

        assert torch.equal(step4(), contiguous()), (label, ps)     # the same bits, before anything is timed
        variants[f"paged fp4 {ps}"] = step4
        variants[f"paged fp8 {ps}"] = step8
    torch.cuda.synchronize()
    t = rounds(variants)
    again = ratios(t["contiguous fp4 again"], t["contiguous fp4"])
    for name in variants:
        kt = kernel_times(variants[name], KERNELS) if not name.endswith("again") else {}
        cols = [f"{kt[n]:.1f}" if n in kt else "" for n in KERNELS]
        r = "" if name == "contiguous fp4" else fmt_ratio(ratios(t[name], t["contiguous fp4"]))
        r8 = fmt_ratio(ratios(t[name], t["paged fp8 " + name.split()[-1]])) if name.startswith("paged fp4") else ""
        emit(f"| {name} | {med(t[name]):.4f} | {r} | {r8} | " + " | ".join(cols) + " |")
        if name.startswith("paged fp4"):
            rs = ratios(t[name], t["contiguous fp4"])
            verdicts.append((label, name, med(rs), min(rs), max(rs), min(again), max(again), r8))
    del ref, keep, variants, q, k, v
    torch.cuda.empty_cache()

emit()
emit("## Paged FP4 step against its two yardsticks")
emit()
emit("| shape | variant | / contiguous fp4 (median, least .. greatest) | contiguous fp4 again / contiguous fp4 | / paged fp8 |")
emit("|---|---|---|---|---|")
for label, name, m, lo, hi, alo, ahi, r8 in verdicts:
    emit(f"| {label} | {name} | {m:.3f}, {lo:.3f} .. {hi:.3f} | {alo:.3f} .. {ahi:.3f} | {r8} |")
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
