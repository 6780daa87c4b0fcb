#!/usr/bin/env python3
"""One decode / chunk step on the paged KV cache WITHOUT fp16 pools -- ``SagePagedRowCache.append_rows`` of the step's T new
rows, then ``sageattn_splitkv_paged`` -- against the same step of ``SagePagedKVCache`` (``append`` after the caller wrote the
rows into its fp16 pools), measured as tools/paged_bench.py measures: ONE process, the variants of a comparison timed round
robin in `--repeats` rounds, each window 3 warm-up calls and HIP events around about `--window-ms` of calls; a time is the
median over the rounds, a ratio the median of the per-round ratios with its least and greatest value.  The step of
``SagePagedKVCache`` is the yardstick and is timed twice per rotation ("bound again"): its spread against itself is what a
difference has to leave behind.

  bound             SagePagedKVCache.append + attention; the new rows already lie in the fp16 pools
  bound + scatter   ... with the scatter of the T new K and V rows into the fp16 pools (two index_put_), which that cache's
                    caller has to do every step
  rows              SagePagedRowCache.append_rows(k_new, v_new) + attention

The four shapes of profiles/paged_kv_cache.md, pages of 64 and 256 keys, a random permutation of all pages as the table.  Every
sequence holds N keys; a step appends the rows [N - T, N) each time.  The first ``rows`` step follows a prepare at N - T rows
and is compared bit for bit with ``bound`` before anything is timed.  The timed repetitions of a chunk that spans more than
one tile boundary (T = 128, 512) lie outside the ring's precondition -- the ring then holds the rows of the last two tiles,
not of the first one -- so they move the same bytes but quantize the first tile from other rows; T = 1 and T = 4 repeat the
legitimate call.  Kernel times: mean device time from a torch.profiler trace of 5 steps, taken after the timing.

usage: paged_rows_bench.py [--repeats 5] [--window-ms 100] [--pv fp16,fp8] [--commit HASH] [--out FILE]"""
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


def nbytes(*tensors):
    return sum(t.numel() * t.element_size() for t in tensors if t is not None)


if not torch.cuda.is_available():
    sys.exit("paged_rows_bench.py measures on the GPU: none is visible")

# (label, (B, Hq, Hk, M, N, D) as the operator sees it, T rows appended per step, q_fold or None: non-causal)
SHAPES = [("(8, 32, 1, 8192, 128) folded by the GQA group 4: q [8, 8, 4, 128], T = 1", (8, 8, 8, 4, 8192, 128), 1, None),
          ("(1, 32, 128, 65536, 128), T = 128", (1, 32, 32, 128, 65536, 128), 128, None),
          ("(1, 40, 512, 32760, 128), T = 512", (1, 40, 40, 512, 32760, 128), 512, None),
          ("causal (8, 8, 16, 8192, 128), q_fold = 4, T = 4", (8, 8, 8, 16, 8192, 128), 4, 4)]
KERNELS = ("kv_cache_append", "attn_i8_splitkv", "splitkv_merge_kernel")

emit("# A paged KV cache without fp16 pools: step times and memory on MI355X")
emit()
emit(f"commit {a.commit or 'unknown'}; tools/paged_rows_bench.py, one process, the variants of a comparison timed round robin in")
emit(f"{a.repeats} rounds, a window = 3 warm-up calls and HIP events around about {a.window_ms:.0f} ms of calls.  fp16 inputs, per-thread")
emit("scales, kv_lens = N for every sequence (on the device), the automatic split count, a random permutation of all pages as the")
emit("table.  \"bound\": SagePagedKVCache.append of the last T rows + sageattn_splitkv_paged -- the parent's code, instruction for")
emit("instruction; \"bound + scatter\": with the two index_put_ that write the T new K and V rows into its fp16 pools first;")
emit("\"rows\": SagePagedRowCache.append_rows(k_new, v_new) + sageattn_splitkv_paged.  Times: median over the rounds.  Ratios: median")
emit("of the per-round ratios (least .. greatest) to \"bound\"; \"bound again\" is the yardstick timed a second time in the same")
emit("rotation.  Kernel columns: mean device time per step from a torch.profiler trace of 5 steps, run after the timing.  Bytes: all")
emit("state of the cache (for \"bound\" with the fp16 pools it binds) over pages x page_size x Hk, so the per-sequence state -- km, the")
emit("V statistics, the ring of 2 x 64 fp16 K rows -- is spread over the keys of the capacity.")
verdicts, memory = [], []
for label, (B, Hq, Hk, M, N, D), T, fold in SHAPES:
    Ncap = (N + 255) // 256 * 256
    S = core.splitkv_num_splits(B, Hq, M, Ncap)
    emit()
    emit(f"## {label}")
    emit()
    emit(f"S = {S} (the automatic choice), capacity {Ncap} keys")
    emit()
    emit("| PV | page | variant | ms | / bound | append us | attention us | merge us |")
    emit("|---|---|---|---|---|---|---|---|")
    g = torch.Generator(device="cuda").manual_seed(1)
    q = torch.randn(B, Hq, M, D, generator=g, device="cuda").half()
    k = (torch.randn(B, Hk, Ncap, D, generator=g, device="cuda") + 0.5 * torch.randn(B, Hk, 1, D, generator=g, device="cuda")).half()
    v = torch.randn(B, Hk, Ncap, D, generator=g, device="cuda").half()
    lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
    start = torch.full((B,), N - T, dtype=torch.int32, device="cuda")
    k_new, v_new = k[:, :, N - T:N].contiguous(), v[:, :, N - T:N].contiguous()
    for pv in a.pv.split(","):
        for ps in (64, 256):
            mp = Ncap // ps
            table = torch.randperm(B * mp, generator=torch.Generator().manual_seed(ps)).to(torch.int32).view(B, mp).cuda()
            k_pool, v_pool = to_pages(k, ps, table), to_pages(v, ps, table)
            # the parent's cache, prepared at N - T rows as the other one, then the step
            bound = sa.SagePagedKVCache.prepare(k_pool, v_pool, table, start, pv=pv)
            rows_cache = sa.SagePagedRowCache.prepare(k[:, :, :N - T], v[:, :, :N - T], table, start, B * mp, ps, pv=pv)
            r = torch.arange(N - T, N, device="cuda")
            pages = table.long()[:, r // ps]                              # [B, T]
            offs = (r % ps).expand(B, T)
            kn, vn = k_new.transpose(1, 2), v_new.transpose(1, 2)         # [B, T, Hk, D]

            def attend(cache, table=table):
                return sa.sageattn_splitkv_paged(q, cache, table, lens, S, causal=fold is not None, q_fold=fold or 1)

            def step_bound(bound=bound, table=table):
                bound.append(table, start, lens, T)
                return attend(bound)

            def step_scatter(bound=bound, table=table, k_pool=k_pool, v_pool=v_pool, pages=pages, offs=offs, kn=kn, vn=vn):
                k_pool[pages, :, offs] = kn
                v_pool[pages, :, offs] = vn
                bound.append(table, start, lens, T)
                return attend(bound)

            def step_rows(rows_cache=rows_cache, table=table):
                rows_cache.append_rows(k_new, v_new, table, start, lens)
                return attend(rows_cache)

            o_rows, o_bound = step_rows(), step_bound()                   # the first, legitimate step: the same bits
            assert torch.equal(o_rows, o_bound), (label, pv, ps)
            assert torch.equal(step_scatter(), o_bound), (label, pv, ps)
            variants = {"bound": step_bound, "bound again": step_bound, "bound + scatter": step_scatter, "rows": step_rows}
            torch.cuda.synchronize()
            t = rounds(variants)
            again = ratios(t["bound again"], t["bound"])
            for name in variants:
                kt = kernel_times(variants[name], KERNELS) if name != "bound again" else {}
                cols = [f"{kt[n]:.1f}" if n in kt else "" for n in KERNELS]
                rr = "" if name == "bound" else fmt_ratio(ratios(t[name], t["bound"]))
                emit(f"| {pv} | {ps} | {name} | {med(t[name]):.4f} | {rr} | " + " | ".join(cols) + " |")
            for name, base in (("rows", "bound"), ("rows", "bound + scatter")):
                rs = ratios(t[name], t[base])
                verdicts.append((label, pv, ps, f"{name} / {base}", med(rs), min(rs), max(rs), min(again), max(again),
                                 min(again) <= med(rs) <= max(again)))
            keys = B * mp * ps * Hk
            b_bound = nbytes(k_pool, v_pool, bound.k8, bound.k_scale, bound.km, bound.v8, bound.v_scale, bound.v_coef)
            memory.append((label, pv, ps, keys, nbytes(k_pool, v_pool), b_bound, rows_cache.nbytes()))
            del bound, rows_cache, variants, k_pool, v_pool
            torch.cuda.empty_cache()
    del q, k, v
    torch.cuda.empty_cache()

emit()
emit("## The step on the cache without fp16 pools against the parent's")
emit()
emit("inside: the median ratio lies within the yardstick's own least .. greatest.")
emit()
emit("| shape | PV | page | ratio | median, least .. greatest | bound again / bound | inside |")
emit("|---|---|---|---|---|---|---|")
for label, pv, ps, what, m, lo, hi, alo, ahi, ok in verdicts:
    emit(f"| {label} | {pv} | {ps} | {what} | {m:.3f}, {lo:.3f} .. {hi:.3f} | {alo:.3f} .. {ahi:.3f} | {'yes' if ok else 'no'} |")
emit()
emit("## Memory: bytes per cached key and KV head (head_dim 128)")
emit()
emit("From the layouts: fp16 cache 512; SagePagedKVCache 640.25 (FP16 P.V) / 768.25 (FP8 P.V) with the pools it binds;")
emit("SagePagedRowCache 384.25 / 256.25 plus the per-sequence state.  Measured (nbytes of every tensor):")
emit()
emit("| shape | PV | page | fp16 pools | SagePagedKVCache + pools | SagePagedRowCache.nbytes() | rows / fp16 | rows / bound |")
emit("|---|---|---|---|---|---|---|---|")
for label, pv, ps, keys, b16, bb, br in memory:
    emit(f"| {label} | {pv} | {ps} | {b16 / keys:.2f} | {bb / keys:.2f} | {br / keys:.2f} | {br / b16:.3f} | {br / bb:.3f} |")
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
