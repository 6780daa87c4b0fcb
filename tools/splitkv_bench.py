#!/usr/bin/env python3
"""``sageattn_splitkv`` (the keys of a q-block spread over several workgroups) measured in ONE process with alternating
windows, as tools/kvlen_bench.py does: every variant of a comparison is timed in turn, `--repeats` times round robin, each
window a warm-up and then HIP events around enough calls to last about `--window-ms`.  A time is the median over the windows;
a ratio is the median of the per-round ratios with their least and greatest value beside it.  Every comparison carries the
dense call a second time ("dense again"): the spread of dense against itself is the yardstick a gain is judged by.

Whole calls (pre-pass + attention [+ merge]) on the same tensors, the dense operator against ``sageattn_splitkv`` with
S in {1, 2, 4, 8, 16} (S = 1 is the dense operator through the new entry) and with the automatic choice:
  (1, 40, 512, 32760, 128)     text / latent queries over a long video context
  (1, 32, 128, 65536, 128)     a speculative chunk over a long cache
  (8, 32, 1, 8192, 128)        a decode step, the 4 query heads of a KV head folded into query rows: q [8, 8, 4, 128]
  (4, 32, 8192, 8192, 128)     the control: the grid fills the chip, the automatic choice must be 1 (S = 2 only beside it)
The attention and the merge kernel of every S are listed separately, from a torch.profiler trace of a few calls.

``--causal``: ``sageattn_splitkv_causal`` (the chunk aligned to the end of the keys) instead, written to
profiles/splitkv_causal.md.  The yardstick is the NON-CAUSAL ``sageattn_splitkv`` of the same shape and S, timed twice per
rotation; only the last T keys differ between the two, so a ratio near 1.0 is what one would suppose:
  (1, 40, 512, 32760, 128)     a chunk of a chunked prefill
  (8, 8, 16, 8192, 128)        a speculative step of 4 tokens, the 4 query heads of a KV head folded into rows (q_fold = 4)
  (1, 8, 64, 4096, 128)        small enough that ``sageattn_qk_int8_pv_fp16_triton`` with the equivalent bool attn_mask -- the
                               only way to this result before -- is timed beside it (FP16 PV only: it has no FP8 form)
There is no pass / fail time: the ratios are reported with the yardstick's spread.

usage: splitkv_bench.py [--causal] [--repeats 5] [--window-ms 100] [--pv fp16,fp8] [--commit HASH] [--out profiles/splitkv.md]"""
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
ap.add_argument("--causal", action="store_true")
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


def kernel_times(fn, calls=5, attn_name="attn_i8_splitkv_kernel", merge_name="splitkv_merge_kernel"):
    """mean device time (us) of the split-KV attention and merge kernels over `calls` calls -> (attn, merge) or None"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        attn = merge = 0.0
        n_attn = n_merge = 0
        for it in prof.key_averages():
            tot = 0.0
            for attr in ("self_device_time_total", "device_time_total", "self_cuda_time_total", "cuda_time_total"):
                tot = getattr(it, attr, 0.0) or 0.0
                if tot:
                    break
            if not tot:
                continue
            if attn_name in it.key:
                attn += tot; n_attn += it.count
            elif merge_name in it.key:
                merge += tot; n_merge += it.count
        if not n_attn or not n_merge:
            return None
        return attn / n_attn, merge / n_merge
    except Exception as exc:  # the trace is a listing beside the timed calls, not one of them
        print(f"(no kernel trace: {exc})", flush=True)
        return None


def make(B, Hq, Hk, M, N, D, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = torch.randn(B, Hq, M, D, generator=g, device="cuda").half()
    k = (torch.randn(B, Hk, N, D, generator=g, device="cuda") + 0.5 * torch.randn(B, Hk, 1, D, generator=g, device="cuda")).half()
    v = torch.randn(B, Hk, N, D, generator=g, device="cuda").half()
    return q, k, v


def dense_of(pv):
    return sa.sageattn_qk_int8_pv_fp16_cuda if pv == "fp16" else sa.sageattn_qk_int8_pv_fp8_cuda


if not torch.cuda.is_available():
    sys.exit("splitkv_bench.py measures on the GPU: none is visible")



def causal_section():
    # (label, (B, Hq, Hk, M, N, D) as the operator sees it, q_fold, beside the masked operator?)
    shapes = [("(1, 40, 512, 32760, 128), a chunk of 512 tokens", (1, 40, 40, 512, 32760, 128), 1, False),
              ("(8, 8, 16, 8192, 128), 4 speculative tokens folded by the GQA group 4", (8, 8, 8, 16, 8192, 128), 4, False),
              ("(1, 8, 64, 4096, 128), beside the masked operator", (1, 8, 8, 64, 4096, 128), 1, True)]
    emit("# sageattn_splitkv_causal: a chunk aligned to the end of the keys, times on MI355X")
    emit()
    emit(f"commit {a.commit or 'unknown'}; tools/splitkv_bench.py --causal, one process, the variants of a comparison timed round robin")
    emit(f"in {a.repeats} rounds, a window = 3 warm-up calls and HIP events around about {a.window_ms:.0f} ms of calls.  fp16 inputs,")
    emit("per-thread scales, no kv_lens (every batch has N keys), whole calls (pre-pass + attention + merge) on the same tensors.")
    emit("Times: median over the rounds.  Ratios: median of the per-round ratios (least .. greatest) to \"non-causal\", the")
    emit("sageattn_splitkv call of the same shape and S.  \"non-causal again\" is that call timed a second time in the same")
    emit("rotation: its ratio is the spread a ratio has to leave before it says anything.  \"attention us\" / \"merge us\": the two")
    emit("kernels of the call alone, mean device time from a torch.profiler trace of 5 calls.  No pass / fail time.")
    notes, slower = [], []
    for label, (B, Hq, Hk, M, N, D), fold, masked in shapes:
        S = core.splitkv_num_splits(B, Hq, M, N)
        emit()
        emit(f"## {label}")
        emit()
        emit(f"q_fold = {fold}: {M // fold} tokens; S = {S} (the automatic choice), grid {B * Hq * ((M + 127) // 128) * S} workgroups")
        emit()
        emit("| PV | variant | ms | / non-causal | attention us | merge us |")
        emit("|---|---|---|---|---|---|")
        q, k, v = make(B, Hq, Hk, M, N, D, 1)
        mask = None
        if masked:  # the band of the rule as the [M, N] bool mask of the masked operator (True = attend)
            tok = torch.arange(M, device="cuda") // fold
            mask = torch.arange(N, device="cuda").view(1, -1) <= (tok + (N - M // fold)).view(-1, 1)
        for pv in a.pv.split(","):
            variants = {"non-causal": lambda: sa.sageattn_splitkv(q, k, v, num_splits=S, pv=pv),
                        "non-causal again": lambda: sa.sageattn_splitkv(q, k, v, num_splits=S, pv=pv),
                        "causal": lambda: sa.sageattn_splitkv_causal(q, k, v, num_splits=S, q_fold=fold, pv=pv)}
            if masked and pv == "fp16":
                variants["sageattn_qk_int8_pv_fp16_triton, bool attn_mask"] = \
                    lambda: sa.sageattn_qk_int8_pv_fp16_triton(q, k, v, attn_mask=mask)
            t = rounds(variants)
            again = ratios(t["non-causal again"], t["non-causal"])
            kts = {}
            for name in variants:
                kt = None
                if name == "causal":
                    kt = kernel_times(variants[name], 5, "attn_i8_splitkv_causal_kernel")
                elif name == "non-causal" and S > 1:
                    kt = kernel_times(variants[name])
                kts[name] = kt
                r = "" if name == "non-causal" else fmt_ratio(ratios(t[name], t["non-causal"]))
                emit(f"| {pv} | {name} | {med(t[name]):.4f} | {r} | {'' if kt is None else f'{kt[0]:.1f}'} | "
                     f"{'' if kt is None else f'{kt[1]:.1f}'} |")
            rc = ratios(t["causal"], t["non-causal"])
            where = "inside" if min(rc) <= max(again) and max(rc) >= min(again) else ("below" if max(rc) < min(again) else "ABOVE")
            notes.append((label, pv, med(rc), min(rc), max(rc), min(again), max(again), where))
            if where == "ABOVE" and kts.get("causal") and kts.get("non-causal"):  # where the time goes: the two kernels apart
                (ca, cm), (na, nm) = kts["causal"], kts["non-causal"]
                slower.append(f"{label}, {pv}: the call is {1e3 * (med(t['causal']) - med(t['non-causal'])):.1f} us slower; its "
                              f"attention kernel takes {ca:.1f} us against {na:.1f} us, its merge {cm:.1f} us against {nm:.1f} us.")
        del q, k, v
        torch.cuda.empty_cache()
    emit()
    emit("## Causal against non-causal")
    emit()
    emit("| shape | PV | causal / non-causal (median, least .. greatest) | non-causal again (least .. greatest) | the causal ratio lies |")
    emit("|---|---|---|---|---|")
    for label, pv, m, lo, hi, alo, ahi, where in notes:
        emit(f"| {label} | {pv} | {m:.3f}, {lo:.3f} .. {hi:.3f} | {alo:.3f} .. {ahi:.3f} | {where} the yardstick's spread |")
    if slower:
        emit()
        emit("Slower than the non-causal call beyond its spread -- where the time goes, from the kernel traces above:")
        emit()
        for line in slower:
            emit("- " + line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if a.causal:
    causal_section()
    sys.exit(0)

# (label, (B, Hq, Hk, M, N, D) as the operator sees it, S values of the sweep)
SHAPES = [("(1, 40, 512, 32760, 128)", (1, 40, 40, 512, 32760, 128), (1, 2, 4, 8, 16)),
          ("(1, 32, 128, 65536, 128)", (1, 32, 32, 128, 65536, 128), (1, 2, 4, 8, 16)),
          ("(8, 32, 1, 8192, 128) folded by the GQA group 4: q [8, 8, 4, 128]", (8, 8, 8, 4, 8192, 128), (1, 2, 4, 8, 16)),
          ("(4, 32, 8192, 8192, 128), the control", (4, 32, 32, 8192, 8192, 128), (1, 2))]

emit("# sageattn_splitkv: the keys of a q-block spread over the chip, times on MI355X")
emit()
emit(f"commit {a.commit or 'unknown'}; tools/splitkv_bench.py, one process, the variants of a comparison timed round robin in {a.repeats}")
emit(f"rounds, a window = 3 warm-up calls and HIP events around about {a.window_ms:.0f} ms of calls.  fp16 inputs, per-thread scales,")
emit("whole calls (pre-pass + attention, with S > 1 + merge) on the same tensors.  Times: median over the rounds.  Ratios:")
emit("median of the per-round ratios (least .. greatest).  \"dense again\" is the dense call timed a second time in the same")
emit("rotation: its ratio to dense is the spread a ratio has to leave before it says anything.  \"attention us\" / \"merge us\": the")
emit("two kernels of the split-KV call alone, mean device time from a torch.profiler trace of 5 calls.")
verdicts = []
for label, (B, Hq, Hk, M, N, D), sweep in SHAPES:
    auto = core.splitkv_num_splits(B, Hq, M, N)
    emit()
    emit(f"## {label}")
    emit()
    emit(f"grid without splits: {B * Hq * ((M + 127) // 128)} workgroups, {(N + 63) // 64} key tiles each; "
         f"automatic choice: S = {auto}")
    emit()
    emit("| PV | variant | ms | / dense | attention us | merge us |")
    emit("|---|---|---|---|---|---|")
    q, k, v = make(B, Hq, Hk, M, N, D, 1)
    for pv in a.pv.split(","):
        dense = dense_of(pv)
        variants = {"dense": lambda: dense(q, k, v), "dense again": lambda: dense(q, k, v)}
        for S in sweep:
            variants[f"S = {S}"] = (lambda S=S: sa.sageattn_splitkv(q, k, v, num_splits=S, pv=pv))
        t = rounds(variants)
        again = ratios(t["dense again"], t["dense"])
        for name in variants:
            kt = None
            if name.startswith("S = ") and name != "S = 1":
                kt = kernel_times(variants[name])
            r = "" if name == "dense" else fmt_ratio(ratios(t[name], t["dense"]))
            mark = "  <- automatic" if name == f"S = {auto}" else ""
            emit(f"| {pv} | {name}{mark} | {med(t[name]):.4f} | {r} | {'' if kt is None else f'{kt[0]:.1f}'} | "
                 f"{'' if kt is None else f'{kt[1]:.1f}'} |")
        if auto > 1:
            ra = ratios(t[f"S = {auto}"], t["dense"])
            # faster than dense by more than dense's own spread: even the slowest round of the automatic call, relative to
            # dense, lies below the fastest "dense again" round
            ok = max(ra) < min(again) and max(ra) < 1.0
            best = min((S for S in sweep), key=lambda S: med(t[f"S = {S}"]))
            verdicts.append((label, pv, auto, med(ra), max(ra), min(again), max(again), ok, best))
        else:
            r1 = ratios(t["S = 1"], t["dense"])
            verdicts.append((label, pv, auto, med(r1), max(r1), min(again), max(again), None, 1))
    del q, k, v
    torch.cuda.empty_cache()

emit()
emit("## The automatic choice")
emit()
emit("Acceptance: wherever the rule picks S > 1, that call is faster than the dense call by more than the dense call's own")
emit("spread -- its slowest round relative to dense lies below the fastest round of \"dense again\" relative to dense.")
emit()
emit("| shape | PV | automatic S | automatic / dense (median, greatest) | dense again / dense (least .. greatest) | fastest S of the sweep | met |")
emit("|---|---|---|---|---|---|---|")
for label, pv, auto, m, mx, lo, hi, ok, best in verdicts:
    met = "n/a (S = 1: the dense launches)" if ok is None else ("yes" if ok else "NO")
    emit(f"| {label} | {pv} | {auto} | {m:.3f}, {mx:.3f} | {lo:.3f} .. {hi:.3f} | {best} | {met} |")
emit()
emit(f"Constants of core.splitkv_num_splits at this measurement: at least {core.SPLITKV_MIN_TILES} key tiles per split, "
     f"{core.SPLITKV_SLOTS} resident workgroup slots, at most {core.SPLITKV_MAX} splits.")
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
