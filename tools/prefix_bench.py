#!/usr/bin/env python3
"""One decode / speculative step of B sequences behind a shared prefix -- ``append_rows`` of the step's T new rows, then
``sageattn_splitkv_paged_prefix`` on ONE quantized copy of the prefix -- against the same step of
``sageattn_splitkv_paged(causal=True)`` with every sequence holding its own copy of the prefix in its own pages, measured as
tools/paged_rows_bench.py measures: ONE process, the variants timed round robin in `--repeats` rounds, each window 3 warm-up
calls and HIP events around about `--window-ms` of calls; a time is the median over the rounds, a ratio the median of the
per-round ratios with its least and greatest value.  The unshared step is the yardstick and is timed twice per rotation
("unshared again"): its spread against itself is what a difference has to leave behind.

Shapes: Hq 32 on Hk 8 folded by the GQA group (q [B, 8, 4 T, 128], q_fold 4), a prefix of Np = 8192 keys, suffixes of Ns = 256
keys after the step, B = 8 and 32 with T = 1 and one speculative shape with T = 4; pages of 256 keys in a random permutation;
both P.V types.  Beside the times: the ratio bytes alone would give, (Np + B Ns) / (B (Np + Ns)); the three kernels' device
times from one torch.profiler trace; the bytes of cache state a sequence saves; and the max abs error of o and lse against
float64 attention over the concatenated keys, for both calls -- the quantization differs, because the shared prefix is
smoothed by its own mean.

usage: prefix_bench.py [--repeats 5] [--window-ms 100] [--pv fp16,fp8] [--commit HASH] [--out FILE]"""
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


def reference(q, k, v, fold, sm_scale):
    """float64 attention of q [B,H,M,D] over k, v [B,H,N,D]: row r is token r // fold, the tokens the last M / fold positions"""
    M, N = q.size(2), k.size(2)
    s = (q.double() @ k.double().transpose(2, 3)) * sm_scale
    tok = torch.arange(M, device=q.device) // fold
    keep = torch.arange(N, device=q.device).view(1, N) <= (N - M // fold + tok).view(M, 1)
    s = s.masked_fill(~keep, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    return torch.exp(s - lse.unsqueeze(-1)) @ v.double(), lse


if not torch.cuda.is_available():
    sys.exit("prefix_bench.py measures on the GPU: none is visible")

HK, G, D, NP, NS, PS = 8, 4, 128, 8192, 256, 256
SHAPES = [(8, 1), (32, 1), (8, 4)]          # (B, T)
KERNELS = ("kv_cache_append", "attn_i8_splitkv_paged", "attn_i8_splitkv_causal_paged", "prefix_merge_kernel",
           "splitkv_merge_kernel")

emit("# Shared-prefix attention on the paged KV cache: step times, bytes and accuracy on MI355X")
emit()
emit(f"commit {a.commit or 'unknown'}; tools/prefix_bench.py, one process, the variants of a comparison timed round robin in")
emit(f"{a.repeats} rounds, a window = 3 warm-up calls and HIP events around about {a.window_ms:.0f} ms of calls.  fp16 inputs, per-thread")
emit(f"scales, Hq 32 on Hk {HK} folded by the GQA group (q [B, {HK}, {G} T, {D}], q_fold {G}), prefix Np = {NP} keys, suffixes Ns = {NS}")
emit(f"keys after the step, pages of {PS} keys in a random permutation, SagePagedRowCache, the automatic split counts.")
emit("\"shared\": append_rows of the T new rows of every suffix + sageattn_splitkv_paged_prefix on one copy of the prefix;")
emit("\"unshared\": the same step of sageattn_splitkv_paged(causal=True) with Np + Ns keys per sequence, each with its own copy of")
emit("the prefix -- the parent's code.  Ratios: median of the per-round ratios (least .. greatest) to \"unshared\"; \"unshared")
emit("again\" is the yardstick timed a second time in the same rotation.  \"bytes bound\": (Np + B Ns) / (B (Np + Ns)), what the K / V")
emit("bytes alone would give; no ratio is promised.  Kernel columns: mean device time per step from a torch.profiler trace of 5")
emit("steps, run after the timing.  Errors: max abs error against float64 attention over the concatenated keys.")
emit()
emit("| B | T | PV | variant | ms | / unshared | bytes bound | append us | prefix pass us | suffix pass us | merge us |")
emit("|---|---|---|---|---|---|---|---|---|---|---|")
memory, errors = [], []
for B, T in SHAPES:
    M = G * T
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda")  # noqa: E731
    q = rnd(B, HK, M, D).half()
    k_p, v_p = (rnd(1, HK, NP, D) + 0.5 * rnd(1, HK, 1, D)).half(), rnd(1, HK, NP, D).half()
    k_s, v_s = (rnd(B, HK, NS, D) + 0.5 * rnd(B, HK, 1, D)).half(), rnd(B, HK, NS, D).half()
    k_u, v_u = torch.cat([k_p.expand(B, -1, -1, -1), k_s], 2), torch.cat([v_p.expand(B, -1, -1, -1), v_s], 2)
    k_new, v_new = k_s[:, :, NS - T:].contiguous(), v_s[:, :, NS - T:].contiguous()
    o_ref, lse_ref = reference(q, k_u, v_u, G, D ** -0.5)
    bound = (NP + B * NS) / (B * (NP + NS))
    for pv in a.pv.split(","):
        mp_p, mp_s, mp_u = NP // PS, NS // PS, (NP + NS) // PS
        perm = torch.randperm(mp_p + B * mp_s, generator=torch.Generator().manual_seed(B)).to(torch.int32).cuda()
        ptable, table = perm[:mp_p].view(1, mp_p).contiguous(), perm[mp_p:].view(B, mp_s).contiguous()
        table_u = torch.randperm(B * mp_u, generator=torch.Generator().manual_seed(B + 1)).to(torch.int32).view(B, mp_u).cuda()
        i32 = lambda n, x: torch.full((n,), x, dtype=torch.int32, device="cuda")  # noqa: E731
        plen, lens, start = i32(1, NP), i32(B, NS), i32(B, NS - T)
        lens_u, start_u = i32(B, NP + NS), i32(B, NP + NS - T)
        whole = sa.SagePagedRowCache.allocate(mp_p + B * mp_s, PS, B + 1, HK, D, torch.float16, "cuda", pv=pv)
        prefix, cache = whole.narrow(0, 1), whole.narrow(1, B)
        prefix.prepare_(k_p, v_p, ptable, plen)
        cache.prepare_(k_s[:, :, :NS - T], v_s[:, :, :NS - T], table, start)
        unshared = sa.SagePagedRowCache.prepare(k_u[:, :, :NP + NS - T], v_u[:, :, :NP + NS - T], table_u, start_u, B * mp_u, PS,
                                                pv=pv)

        def step_shared(cache=cache, prefix=prefix, table=table, ptable=ptable, lens=lens, start=start, plen=plen):
            cache.append_rows(k_new, v_new, table, start, lens)
            return sa.sageattn_splitkv_paged_prefix(q, cache, table, lens, prefix, ptable, plen, q_fold=G, return_lse=True)

        def step_unshared(unshared=unshared, table_u=table_u, lens_u=lens_u, start_u=start_u):
            unshared.append_rows(k_new, v_new, table_u, start_u, lens_u)
            return sa.sageattn_splitkv_paged(q, unshared, table_u, lens_u, causal=True, q_fold=G, return_lse=True)

        (o_s, l_s), (o_u, l_u) = step_shared(), step_unshared()
        torch.cuda.synchronize()
        errors.append((B, T, pv, (o_s.double() - o_ref).abs().max().item(), (l_s.double() - lse_ref).abs().max().item(),
                       (o_u.double() - o_ref).abs().max().item(), (l_u.double() - lse_ref).abs().max().item()))
        Sp, Ss = core.splitkv_num_splits(1, HK, B * M, NP), core.splitkv_num_splits(B, HK, M, NS)
        Su = core.splitkv_num_splits(B, HK, M, NP + NS)
        variants = {"unshared": step_unshared, "unshared again": step_unshared, "shared": step_shared}
        t = rounds(variants)
        for name in variants:
            kt = kernel_times(variants[name], KERNELS) if name != "unshared again" else {}
            merge = kt.get("prefix_merge_kernel", kt.get("splitkv_merge_kernel"))
            cols = [kt.get("kv_cache_append"), kt.get("attn_i8_splitkv_paged"), kt.get("attn_i8_splitkv_causal_paged"), merge]
            rr = "" if name == "unshared" else fmt_ratio(ratios(t[name], t["unshared"]))
            splits = f" (Sp {Sp}, Ss {Ss})" if name == "shared" else f" (S {Su})" if name == "unshared" else ""
            emit(f"| {B} | {T} | {pv} | {name}{splits} | {med(t[name]):.4f} | {rr} | {bound:.3f} | "
                 + " | ".join("" if c is None else f"{c:.1f}" for c in cols) + " |")
        memory.append((B, T, pv, whole.nbytes(), unshared.nbytes()))
        del whole, prefix, cache, unshared, variants
        torch.cuda.empty_cache()

emit()
emit("## Bytes of cache state")
emit()
emit("| B | T | PV | shared: all state | unshared: all state | saved per sequence | shared / unshared |")
emit("|---|---|---|---|---|---|---|")
for B, T, pv, bs, bu in memory:
    emit(f"| {B} | {T} | {pv} | {bs} | {bu} | {(bu - bs) / B:.0f} | {bs / bu:.3f} |")
emit()
emit("## Max abs error against float64 attention over the concatenated keys (reported, not asserted)")
emit()
emit("| B | T | PV | shared: o | shared: lse | unshared: o | unshared: lse |")
emit("|---|---|---|---|---|---|---|")
for B, T, pv, eo, el, uo, ul in errors:
    emit(f"| {B} | {T} | {pv} | {eo:.3e} | {el:.3e} | {uo:.3e} | {ul:.3e} |")
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
