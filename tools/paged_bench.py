#!/usr/bin/env python3
"""One decode / chunk step on the PAGED KV cache -- ``SagePagedKVCache.append`` of T rows, then ``sageattn_splitkv_paged`` --
against the same step of the contiguous ``SageKVCache`` on the padded tensors gathered from the pages, measured as
tools/kvcache_bench.py measures: ONE process, the variants of a comparison timed round robin in `--repeats` rounds, each window
3 warm-up calls and HIP events around about `--window-ms` of calls; a time is the median over the rounds, a ratio the median of
the per-round ratios with its least and greatest value.  The contiguous step is the yardstick and is timed twice per rotation
("contiguous again"): its spread against itself is what a difference has to leave behind.

  (8, 32, 1, 8192, 128) folded by the GQA group 4: q [8, 8, 4, 128]      a decode step, T = 1
  (1, 32, 128, 65536, 128)                                               a speculative chunk over a long cache, T = 128
  (1, 40, 512, 32760, 128)                                               text / latent queries over a video context, T = 512
  causal (8, 8, 16, 8192, 128), q_fold = 4                               4 speculative tokens, T = 4

Paged variants: page_size 64 and 256, each with an identity table (sequence b owns the pages b * max_pages ..) and with a
random permutation of all pages.  Every batch holds N keys; the step appends the rows [N - T, N) each time, so that every
timed call is the same call.  Kernel times: mean device time from a torch.profiler trace of 5 steps, taken after the timing.

usage: paged_bench.py [--repeats 5] [--window-ms 100] [--pv fp16,fp8] [--commit HASH] [--append FILE] [--out FILE]"""
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
ap.add_argument("--pv", default="fp16,fp8")
ap.add_argument("--commit", default="")
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


def to_pages(x, page_size, table):
    """the padded [B,Hk,Ncap,D] tensor cut into pages: pool [P,Hk,page_size,D] with page table[b, i] = rows i * page_size .."""
    B, Hk, Ncap, D = x.shape
    mp = Ncap // page_size
    pool = torch.empty((B * mp, Hk, page_size, D), dtype=x.dtype, device=x.device)
    pool[table.reshape(-1).long()] = x.view(B, Hk, mp, page_size, D).permute(0, 2, 1, 3, 4).reshape(B * mp, Hk, page_size, D)
    return pool


if not torch.cuda.is_available():
    sys.exit("paged_bench.py measures on the GPU: none is visible")

# (label, (B, Hq, Hk, M, N, D) as the operator sees it, T rows appended per step, q_fold or None: non-causal)
SHAPES = [("(8, 32, 1, 8192, 128) folded by the GQA group 4: q [8, 8, 4, 128], T = 1", (8, 8, 8, 4, 8192, 128), 1, None),
          ("(1, 32, 128, 65536, 128), T = 128", (1, 32, 32, 128, 65536, 128), 128, None),
          ("(1, 40, 512, 32760, 128), T = 512", (1, 40, 40, 512, 32760, 128), 512, None),
          ("causal (8, 8, 16, 8192, 128), q_fold = 4, T = 4", (8, 8, 8, 16, 8192, 128), 4, 4)]
KERNELS = ("kv_cache_append", "attn_i8_splitkv", "splitkv_merge_kernel")
PAGED = [(ps, kind) for ps in (64, 256) for kind in ("identity", "permuted")]

emit("# A paged quantized KV cache for the split-KV operators: step times on MI355X")
emit()
emit(f"commit {a.commit or 'unknown'}; tools/paged_bench.py, one process, the variants of a comparison timed round robin in")
emit(f"{a.repeats} rounds, a window = 3 warm-up calls and HIP events around about {a.window_ms:.0f} ms of calls.  fp16 inputs, per-thread")
emit("scales, kv_lens = N for every batch (on the device), the automatic split count.  \"contiguous\": SageKVCache.append of the")
emit("last T rows + sageattn_splitkv_cached on the padded tensors (capacity = N rounded up to 256 keys) -- the parent's code,")
emit("instruction for instruction.  \"paged\": SagePagedKVCache.append + sageattn_splitkv_paged on the same rows cut into pages of")
emit("64 or 256 keys, the table the identity or a random permutation of all pages.  Times: median over the rounds.  Ratios: median")
emit("of the per-round ratios (least .. greatest) to \"contiguous\"; \"contiguous again\" is the yardstick timed a second time in the")
emit("same rotation.  Kernel columns: mean device time per step from a torch.profiler trace of 5 steps, run after the timing.")
verdicts = []
for label, (B, Hq, Hk, M, N, D), T, fold in SHAPES:
    Ncap = (N + 255) // 256 * 256
    S = core.splitkv_num_splits(B, Hq, M, Ncap)
    emit()
    emit(f"## {label}")
    emit()
    emit(f"S = {S} (the automatic choice), capacity {Ncap} keys")
    emit()
    emit("| PV | variant | ms | / contiguous | append us | attention us | merge us |")
    emit("|---|---|---|---|---|---|---|")
    g = torch.Generator(device="cuda").manual_seed(1)
    q = torch.randn(B, Hq, M, D, generator=g, device="cuda").half()
    k = (torch.randn(B, Hk, Ncap, D, generator=g, device="cuda") + 0.5 * torch.randn(B, Hk, 1, D, generator=g, device="cuda")).half()
    v = torch.randn(B, Hk, Ncap, D, generator=g, device="cuda").half()
    lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
    start = torch.full((B,), N - T, dtype=torch.int32, device="cuda")
    for pv in a.pv.split(","):
        ref = sa.SageKVCache.prepare(k, v, lens, pv=pv)

        def contiguous():
            ref.append(start, lens, T)
            return sa.sageattn_splitkv_cached(q, ref, lens, S, causal=fold is not None, q_fold=fold or 1)

        variants = {"contiguous": contiguous, "contiguous again": contiguous}
        keep = []
        for ps, kind in PAGED:
            mp = Ncap // ps
            ids = torch.arange(B * mp) if kind == "identity" else torch.randperm(B * mp, generator=torch.Generator().manual_seed(ps))
            table = ids.to(torch.int32).view(B, mp).cuda()
            cache = sa.SagePagedKVCache.prepare(to_pages(k, ps, table), to_pages(v, ps, table), table, lens, pv=pv)
            keep.append(cache)

            def step(cache=cache, table=table):
                cache.append(table, start, lens, T)
                return sa.sageattn_splitkv_paged(q, cache, table, lens, S, causal=fold is not None, q_fold=fold or 1)

            assert torch.equal(step(), contiguous()), (label, pv, ps, kind)     # the same bits, before anything is timed
            variants[f"paged {ps} {kind}"] = step
        torch.cuda.synchronize()
        t = rounds(variants)
        again = ratios(t["contiguous again"], t["contiguous"])
        for name in variants:
            kt = kernel_times(variants[name], KERNELS) if name != "contiguous again" else {}
            cols = [f"{kt[n]:.1f}" if n in kt else "" for n in KERNELS]
            r = "" if name == "contiguous" else fmt_ratio(ratios(t[name], t["contiguous"]))
            emit(f"| {pv} | {name} | {med(t[name]):.4f} | {r} | " + " | ".join(cols) + " |")
            if name.startswith("paged"):
                rs = ratios(t[name], t["contiguous"])
                verdicts.append((label, pv, name, med(rs), min(rs), max(rs), min(again), max(again),
                                 min(again) <= med(rs) <= max(again)))
        del ref, keep, variants
        torch.cuda.empty_cache()
    del q, k, v
    torch.cuda.empty_cache()

emit()
emit("## Paged step against the contiguous step")
emit()
emit("inside: the median ratio lies within the yardstick's own least .. greatest.")
emit()
emit("| shape | PV | variant | paged / contiguous (median, least .. greatest) | contiguous again / contiguous | inside |")
emit("|---|---|---|---|---|---|")
for label, pv, name, m, lo, hi, alo, ahi, ok in verdicts:
    emit(f"| {label} | {pv} | {name} | {m:.3f}, {lo:.3f} .. {hi:.3f} | {alo:.3f} .. {ahi:.3f} | {'yes' if ok else 'no'} |")
if a.append and os.path.exists(a.append):
    emit()
    emit(open(a.append).read().rstrip())
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
