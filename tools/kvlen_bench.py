#!/usr/bin/env python3
"""``sageattn_kvlen`` (per-batch key lengths on the dense padded layout) measured in ONE process with alternating windows:
every variant of a comparison is timed in turn, `--repeats` times round robin, each window a warm-up and then HIP events
around enough calls to last about `--window-ms`.  A time is the median over the windows; a ratio is the median of the
per-round ratios with their least and greatest value beside it.  Every comparison carries the dense call a second time
("dense again"): the spread of dense against itself is the yardstick an overhead is judged by.

  (a) full lengths against dense: kv_lens = N everywhere, (4,32,8192,128) and (4,32,2048,64), FP16 and FP8 PV
  (b) ragged lengths [8192,6144,4096,2048] at (4,32,8192,128): time over the dense time beside sum(len)/(B*N) = 0.625
  (c) cross-attention: (4,40,8192,128) queries on 512 keys with lengths [512,300,130,77]: sageattn_kvlen against
      sageattn_qk_int8_pv_fp16_triton with the equivalent bool [B,1,1,N] mask and against the dense call on all 512 keys
  (d) the dense path: `python bench.py` figures of the parent commit and of this one, taken alternately on one machine by the
      caller and handed in as files of JSON lines (--bench-parent, --bench-branch); absent, the section says "not measured"
Random inputs; rows >= len_b of K and V hold NaN in (b) and (c), as a padded batch may.

usage: kvlen_bench.py [--repeats 5] [--window-ms 250] [--sections a,b,c] [--bench-parent p.jsonl --bench-branch b.jsonl]
                      [--commit HASH] [--out profiles/kvlen.md]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import sageattention_amd as sa  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--window-ms", type=float, default=250.0)
ap.add_argument("--sections", default="a,b,c")
ap.add_argument("--bench-parent", default="")
ap.add_argument("--bench-branch", default="")
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
        calls[name] = max(10, int(a.window_ms / max(events(fn, 5), 1e-3)))
    out = {name: [] for name in variants}
    for _ in range(a.repeats):
        for name, fn in variants.items():
            for _ in range(3):
                fn()
            out[name].append(events(fn, calls[name]))
    return out


def med(ts):
    return statistics.median(ts)


def ratio(ts, base):
    """median of the per-round ratios ts[i] / base[i], with their least and greatest value"""
    r = [x / y for x, y in zip(ts, base)]
    return f"{med(r):.3f} ({min(r):.3f} .. {max(r):.3f})"


def make(B, H, M, N, D, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = torch.randn(B, H, M, D, generator=g, device="cuda").half()
    k = torch.randn(B, H, N, D, generator=g, device="cuda").half()
    v = torch.randn(B, H, N, D, generator=g, device="cuda").half()
    return q, k, v


def poison(k, v, lens):
    for b, n in enumerate(lens):
        k[b, :, n:] = float("nan")
        v[b, :, n:] = float("nan")


def dense_of(pv):
    return sa.sageattn_qk_int8_pv_fp16_cuda if pv == "fp16" else sa.sageattn_qk_int8_pv_fp8_cuda


def bench_lines(path):
    out = []
    for ln in open(path):
        ln = ln.strip()
        if ln.startswith("{"):
            out.append(json.loads(ln))
    return out


if not torch.cuda.is_available():
    sys.exit("kvlen_bench.py measures on the GPU: none is visible")
sections = a.sections.split(",")
emit("# sageattn_kvlen: per-batch key lengths on the dense fast path, times on MI355X")
emit()
emit(f"commit {a.commit or 'unknown'}; tools/kvlen_bench.py, one process, the variants of a comparison timed round robin in {a.repeats}")
emit(f"rounds, a window = 3 warm-up calls and HIP events around about {a.window_ms:.0f} ms of calls.  fp16 inputs, per-thread scales,")
emit("whole calls (pre-pass + attention).  Times: median over the rounds.  Ratios: median of the per-round ratios (least ..")
emit("greatest).  \"dense again\" is the dense call timed a second time in the same rotation: its ratio to dense is the spread a")
emit("ratio has to leave before it says anything.")

if "a" in sections:
    emit()
    emit("## (a) full lengths against dense")
    emit()
    emit("kv_lens = N for every batch; o and lse of the two calls are compared bit for bit first.")
    emit()
    emit("| shape (B,H,N,D) | PV | dense ms | kvlen ms | kvlen / dense | dense again / dense | bits |")
    emit("|---|---|---|---|---|---|---|")
    for (B, H, N, D) in ((4, 32, 8192, 128), (4, 32, 2048, 64)):
        q, k, v = make(B, H, N, N, D, N + D)
        full = torch.full((B,), N, dtype=torch.int32, device="cuda")
        for pv in ("fp16", "fp8"):
            dense = dense_of(pv)
            o0, l0 = dense(q, k, v, return_lse=True)
            o1, l1 = sa.sageattn_kvlen(q, k, v, full, pv=pv, return_lse=True)
            same = "equal" if torch.equal(o0, o1) and torch.equal(l0, l1) else "DIFFERENT"
            del o0, l0, o1, l1
            t = rounds({"dense": lambda: dense(q, k, v), "kvlen": lambda: sa.sageattn_kvlen(q, k, v, full, pv=pv),
                        "again": lambda: dense(q, k, v)})
            emit(f"| ({B},{H},{N},{D}) | {pv} | {med(t['dense']):.4f} | {med(t['kvlen']):.4f} | {ratio(t['kvlen'], t['dense'])} | "
                 f"{ratio(t['again'], t['dense'])} | {same} |")
        del q, k, v

if "b" in sections:
    emit()
    emit("## (b) ragged lengths")
    emit()
    B, H, N, D = 4, 32, 8192, 128
    lens = [8192, 6144, 4096, 2048]
    emit(f"({B},{H},{N},{D}), kv_lens = {lens}: sum(len) / (B N) = {sum(lens) / (B * N):.3f} of the dense call's tiles.  The dense call")
    emit("runs on the same shape with finite K and V (it would attend the padding).")
    emit()
    emit("| PV | dense ms | kvlen ragged ms | ragged / dense | dense again / dense |")
    emit("|---|---|---|---|---|")
    q, k, v = make(B, H, N, N, D, 7)
    kp, vp = k.clone(), v.clone()
    poison(kp, vp, lens)
    kv_lens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    for pv in ("fp16", "fp8"):
        dense = dense_of(pv)
        t = rounds({"dense": lambda: dense(q, k, v), "kvlen": lambda: sa.sageattn_kvlen(q, kp, vp, kv_lens, pv=pv),
                    "again": lambda: dense(q, k, v)})
        emit(f"| {pv} | {med(t['dense']):.4f} | {med(t['kvlen']):.4f} | {ratio(t['kvlen'], t['dense'])} | {ratio(t['again'], t['dense'])} |")
    del q, k, v, kp, vp

if "c" in sections:
    emit()
    emit("## (c) cross-attention")
    emit()
    B, H, M, N, D = 4, 40, 8192, 512, 128
    lens = [512, 300, 130, 77]
    emit(f"({B},{H},{M},{D}) queries on N = {N} keys, kv_lens = {lens}.  masked = sageattn_qk_int8_pv_fp16_triton with the bool")
    emit("[B,1,1,N] mask `arange(N) < len_b` on K and V whose padding rows are zeros (its pre-pass reads them; NaN there would")
    emit("destroy its output); kvlen runs on K and V whose padding rows hold NaN.  dense = sageattn_qk_int8_pv_fp16_cuda on all")
    emit("512 keys (another result: it attends the padding).")
    emit()
    q, k, v = make(B, H, M, N, D, 11)
    kz, vz, kp, vp = k.clone(), v.clone(), k.clone(), v.clone()
    for b, n in enumerate(lens):
        kz[b, :, n:] = 0
        vz[b, :, n:] = 0
    poison(kp, vp, lens)
    kv_lens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    mask = (torch.arange(N, device="cuda").view(1, 1, 1, N) < kv_lens.view(B, 1, 1, 1))
    t = rounds({"masked": lambda: sa.sageattn_qk_int8_pv_fp16_triton(q, kz, vz, attn_mask=mask),
                "kvlen": lambda: sa.sageattn_kvlen(q, kp, vp, kv_lens, pv="fp16"),
                "kvlen8": lambda: sa.sageattn_kvlen(q, kp, vp, kv_lens, pv="fp8"),
                "dense": lambda: sa.sageattn_qk_int8_pv_fp16_cuda(q, k, v),
                "again": lambda: sa.sageattn_qk_int8_pv_fp16_triton(q, kz, vz, attn_mask=mask)})
    om = sa.sageattn_qk_int8_pv_fp16_triton(q, kz, vz, attn_mask=mask).float()
    ok = sa.sageattn_kvlen(q, kp, vp, kv_lens, pv="fp16").float()
    emit("| variant | ms | / masked | / dense |")
    emit("|---|---|---|---|")
    for name, label in (("masked", "masked (attn_mask)"), ("kvlen", "sageattn_kvlen, FP16 PV"), ("kvlen8", "sageattn_kvlen, FP8 PV"),
                        ("dense", "dense, all 512 keys"), ("again", "masked again")):
        emit(f"| {label} | {med(t[name]):.4f} | {ratio(t[name], t['masked'])} | {ratio(t[name], t['dense'])} |")
    emit()
    emit(f"max |kvlen - masked| over the outputs: {float((ok - om).abs().max()):.3e} (two quantizations of K: the masked operator takes")
    emit("its smoothing mean and block scales over all 512 rows).")
    slower = med([x / y for x, y in zip(t["kvlen"], t["masked"])]) > 1.0
    emit()
    emit("The one condition -- sageattn_kvlen not slower than the masked operator on the same problem -- is "
         + ("NOT MET: sageattn_kvlen is SLOWER here." if slower else "met."))
    del q, k, v, kz, vz, kp, vp

emit()
emit("## (d) the dense path: bench.py on the parent commit and on this one")
emit()
if a.bench_parent and a.bench_branch:
    par, br = bench_lines(a.bench_parent), bench_lines(a.bench_branch)
    key = "value"
    emit(f"`python bench.py --gpus 1` run alternately (parent, branch, parent, ...) on one machine, {len(par)} runs each; the JSON")
    emit(f"line's `{key}` ({par[0].get('unit', '')}, {par[0].get('metric', par[0].get('name', 'headline'))}):")
    emit()
    emit("| run | parent | branch |")
    emit("|---|---|---|")
    for i, (x, y) in enumerate(zip(par, br)):
        emit(f"| {i + 1} | {x[key]} | {y[key]} |")
    pv_, bv_ = [x[key] for x in par], [y[key] for y in br]
    emit(f"| median | {med(pv_):.2f} | {med(bv_):.2f} |")
    emit()
    emit(f"parent's own spread: {min(pv_)} .. {max(pv_)} ({(max(pv_) - min(pv_)) / med(pv_) * 100:.2f} % of its median); branch median / parent")
    emit(f"median = {med(bv_) / med(pv_):.4f}.")
else:
    emit("not measured in this run (no --bench-parent / --bench-branch files).")

if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
