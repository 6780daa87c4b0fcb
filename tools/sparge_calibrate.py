#!/usr/bin/env python3
"""Calibration of the block-map predictor, measured and applied (sageattn_tile_mass, plan_recall, sparge_tune), in ONE
process with HIP events and alternating windows.  Writes profiles/sparge_calibration.md.

  1. sageattn_tile_mass beside the dense operator (sageattn_qk_int8_pv_fp16_cuda) at each shape of `--shapes`: the two calls
     alternate, `--repeats` windows of `--launches` calls each, median and spread.  Both times include the K pre-pass and
     the Q quantizer (the dense call folds the latter into its kernel).
  2. one sparge_tune(steps=8) with the mass given and with the mass computed inside.
  3. on the clustered inputs of tests/sparge_util.py (the generator at scale) and on random normal Q / K: recall (mean over
     query rows, min over q-blocks) and density of the predictor at cdfthreshd 0.9 / 0.95 / 0.98, and the per-head cdfthreshd
     and topk that sparge_tune finds for target 0.95.
SYNTHETIC data: the recalls and tuned values describe these generators, not a model.

With --kv-lens the twins with per-batch key lengths instead (sageattn_tile_mass_kvlen, sparge_tune_kvlen), at (4,32,8192,128)
and (4,32,2048,64); writes profiles/sparge_calibration_kvlen.md:
  a. sageattn_tile_mass_kvlen with every length N beside sageattn_tile_mass, the latter timed twice per rotation: its two
     columns against each other are the yardstick.
  b. lengths [N, 3N/4, N/2, N/4] (0.625 of the tiles) as a ratio to the call with full lengths.
  c. sparge_tune_kvlen beside sparge_tune with every length N, the mass computed inside.

usage: sparge_calibrate.py [--launches 50] [--repeats 5] [--shapes c3,c3d64,wan] [--data-shape small] [--commit HASH]
                           [--out profiles/sparge_calibration.md] [--kv-lens]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import sageattention_amd as sa  # noqa: E402

SHAPES = {"c3": (4, 32, 8192, 128), "c3d64": (4, 32, 8192, 64), "wan": (1, 40, 32760, 128), "small": (2, 8, 4096, 128)}
KVLEN_SHAPES = ((4, 32, 8192, 128), (4, 32, 2048, 64))
PROFILES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=50)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--shapes", default="c3,c3d64,wan")
ap.add_argument("--data-shape", default="small")
ap.add_argument("--simthreshd1", type=float, default=0.6)
ap.add_argument("--commit", default="")
ap.add_argument("--kv-lens", action="store_true", help="measure the twins with per-batch key lengths instead")
ap.add_argument("--out", default=None, help="default: profiles/sparge_calibration.md, with --kv-lens "
                                            "profiles/sparge_calibration_kvlen.md")
a = ap.parse_args()
if a.out is None:
    a.out = os.path.join(PROFILES, "sparge_calibration_kvlen.md" if a.kv_lens else "sparge_calibration.md")
lines = []


def emit(s=""):
    print(s, flush=True)
    lines.append(s)


def clustered(B, H, n, D, blk, noise_every, offset, gen):
    nb = (n + blk - 1) // blk
    c = torch.randn(B, H, nb, 1, D, generator=gen, device="cuda") * 2.0
    noisy = (torch.arange(nb, device="cuda") % noise_every == noise_every - 1).view(1, 1, nb, 1, 1)
    c = torch.where(noisy, torch.zeros_like(c), c)
    x = c + torch.randn(B, H, nb, blk, D, generator=gen, device="cuda")
    return (x.reshape(B, H, nb * blk, D)[:, :, :n] + offset).half().contiguous()


def window(fn, n):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n  # ms per call


def spread(ts):
    return f"median {statistics.median(ts):.3f} ms, min {min(ts):.3f}, max {max(ts):.3f}"


def fmt(t, nd=3):
    return "[" + ", ".join(f"{x:.{nd}f}" for x in t.tolist()) + "]"


def write_out():
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def rotate(fns, launches):
    """``a.repeats`` rotations over ``fns`` (name -> call), one window of ``launches`` calls each -> name -> [ms per call]"""
    ts = {n: [] for n in fns}
    for _ in range(a.repeats):
        for n, fn in fns.items():
            ts[n].append(window(fn, launches))
    return ts


def ratio_spread(num, den):
    """median, min and max over the rotations of num / den, window by window"""
    r = [x / y for x, y in zip(num, den)]
    return f"{statistics.median(r):.3f} ({min(r):.3f} .. {max(r):.3f})"


def kvlen_report():
    emit("# Calibration with per-batch key lengths: sageattn_tile_mass_kvlen, sparge_tune_kvlen (MI355X)")
    emit()
    emit(f"commit {a.commit or 'unknown'}; tools/sparge_calibrate.py --kv-lens, HIP events, one process, {a.repeats} rotations of")
    emit(f"alternating windows, {a.launches} calls each (sparge_tune: 5).  fp16, per-thread scales, random normal Q / K, whole calls")
    emit("with their K pre-pass and Q quantizer.  Ratios are taken window by window within a rotation: median (min .. max).")
    emit()
    rows_a, rows_b, rows_c = [], [], []
    for B, H, N, D in KVLEN_SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(N + D)
        q, k = (torch.randn(B, H, N, D, generator=gen, device="cuda").half() for _ in range(2))
        full = torch.full((B,), N, dtype=torch.int32, device="cuda")
        part = torch.tensor([N, 3 * N // 4, N // 2, N // 4], dtype=torch.int32, device="cuda")
        assert torch.equal(sa.sageattn_tile_mass_kvlen(q, k, full), sa.sageattn_tile_mass(q, k)), "full lengths: the same bits"
        ts = rotate({"plain": lambda: sa.sageattn_tile_mass(q, k), "full": lambda: sa.sageattn_tile_mass_kvlen(q, k, full),
                     "plain2": lambda: sa.sageattn_tile_mass(q, k), "part": lambda: sa.sageattn_tile_mass_kvlen(q, k, part)},
                    a.launches)
        shape = f"{(B, H, N, D)}"
        rows_a.append(f"| {shape} | {spread(ts['plain'])} | {spread(ts['plain2'])} | {spread(ts['full'])} | "
                      f"{ratio_spread(ts['plain2'], ts['plain'])} | {ratio_spread(ts['full'], ts['plain'])} |")
        tiles = float(((part + 63) // 64).sum()) / (B * ((N + 63) // 64))
        rows_b.append(f"| {shape} | {part.tolist()} | {tiles:.3f} | {spread(ts['part'])} | {ratio_spread(ts['part'], ts['full'])} |")
        kw = dict(simthreshd1=a.simthreshd1, steps=8)
        t0, t1 = sa.sparge_tune(q, k, **kw), sa.sparge_tune_kvlen(q, k, full, **kw)
        assert all(torch.equal(getattr(t0, n), getattr(t1, n)) for n in ("param", "met", "recall", "recall_below", "density"))
        tt = rotate({"plain": lambda: sa.sparge_tune(q, k, **kw), "full": lambda: sa.sparge_tune_kvlen(q, k, full, **kw),
                     "plain2": lambda: sa.sparge_tune(q, k, **kw)}, 5)
        rows_c.append(f"| {shape} | {spread(tt['plain'])} | {spread(tt['plain2'])} | {spread(tt['full'])} | "
                      f"{ratio_spread(tt['plain2'], tt['plain'])} | {ratio_spread(tt['full'], tt['plain'])} |")
        del q, k
        torch.cuda.empty_cache()
    emit("## a. full lengths: sageattn_tile_mass_kvlen beside sageattn_tile_mass")
    emit()
    emit("Every length is N; the mass is bit-identical to the call without lengths (asserted).  The plain call is timed twice per")
    emit("rotation; its second column over its first is the yardstick for the last column.")
    emit()
    emit("| shape (B, H, N, D) | sageattn_tile_mass | sageattn_tile_mass again | sageattn_tile_mass_kvlen, full | again / plain | kvlen / plain |")
    emit("|---|---|---|---|---|---|")
    for r in rows_a:
        emit(r)
    emit()
    emit("## b. lengths [N, 3N/4, N/2, N/4]")
    emit()
    emit("| shape (B, H, N, D) | kv_lens | share of the tiles | sageattn_tile_mass_kvlen | / the call with full lengths |")
    emit("|---|---|---|---|---|")
    for r in rows_b:
        emit(r)
    emit()
    emit("## c. full lengths: sparge_tune_kvlen beside sparge_tune (steps=8, rule=\"cdf\", the mass computed inside)")
    emit()
    emit("Every field of the result is bit-identical (asserted).")
    emit()
    emit("| shape (B, H, N, D) | sparge_tune | sparge_tune again | sparge_tune_kvlen, full | again / plain | kvlen / plain |")
    emit("|---|---|---|---|---|---|")
    for r in rows_c:
        emit(r)
    write_out()


if a.kv_lens:
    kvlen_report()
    sys.exit(0)

emit("# Calibrating the block-map predictor: exact tile mass, recall, tuned thresholds (MI355X)")
emit()
emit(f"commit {a.commit or 'unknown'}; tools/sparge_calibrate.py, HIP events, one process, {a.repeats} alternating windows of")
emit(f"{a.launches} calls each.  fp16, per-thread scales, simthreshd1 = {a.simthreshd1}.")
emit()
emit("## 1. sageattn_tile_mass beside the dense operator")
emit()
emit("Both columns are whole calls: K pre-pass (mean + INT8 K), Q quantizer, then the kernel.  The tile-mass kernel does the")
emit("QK^T work of the dense kernel twice and two exponentials per score, and no P.V.")
emit()
emit("| shape (B, H, N, D) | sageattn_tile_mass | dense sageattn_qk_int8_pv_fp16_cuda | tile mass / dense (medians) |")
emit("|---|---|---|---|")
for sname in a.shapes.split(","):
    B, H, N, D = SHAPES[sname]
    gen = torch.Generator(device="cuda").manual_seed(N + D)
    q, k, v = (torch.randn(B, H, N, D, generator=gen, device="cuda").half() for _ in range(3))
    fns = {"mass": lambda: sa.sageattn_tile_mass(q, k), "dense": lambda: sa.sageattn_qk_int8_pv_fp16_cuda(q, k, v)}
    ts = {n: [] for n in fns}
    for _ in range(a.repeats):
        for n, fn in fns.items():
            ts[n].append(window(fn, a.launches))
    ratio = statistics.median(ts["mass"]) / statistics.median(ts["dense"])
    emit(f"| {sname} {(B, H, N, D)} | {spread(ts['mass'])} | {spread(ts['dense'])} | {ratio:.2f} |")
    if sname == a.shapes.split(",")[0]:
        mass = sa.sageattn_tile_mass(q, k)
        t_given = [window(lambda: sa.sparge_tune(q, k, simthreshd1=a.simthreshd1, steps=8, mass=mass), 5) for _ in range(a.repeats)]
        t_whole = [window(lambda: sa.sparge_tune(q, k, simthreshd1=a.simthreshd1, steps=8), 5) for _ in range(a.repeats)]
        tune_line = (f"sparge_tune(steps=8, rule=\"cdf\") at {sname} {(B, H, N, D)}: mass given {spread(t_given)}; computing the mass "
                     f"{spread(t_whole)}; dense call {statistics.median(ts['dense']):.3f} ms.")
        del mass
    del q, k, v
    torch.cuda.empty_cache()
emit()
emit("## 2. one sparge_tune")
emit()
emit(tune_line)
emit("Nine selections and nine recall launches plus [Hq] reductions; no host synchronisation inside.")
emit()
emit("## 3. recall of the predictor and tuned thresholds")
emit()
B, H, N, D = SHAPES[a.data_shape]
emit(f"(B, H, N, D) = {(B, H, N, D)}.  recall mean = mean captured probability per query row over all heads; min = the worst")
emit("q-block.  Tuned values per head for target 0.95, reduce=\"mean\", steps=8; SYNTHETIC inputs.  A density of 1.000 at every")
emit("threshold means that no block passed simthreshd1 (rows of random normal blocks are not alike: mean cosine about 1 / rows),")
emit("so every tile is forced on, the parameter selects nothing and the smallest grid value already meets the target.")
gen = torch.Generator(device="cuda").manual_seed(N + D)
data = {"clustered (tests/sparge_util.py's generator)": (clustered(B, H, N, D, 128, 4, 0.0, gen), clustered(B, H, N, D, 64, 5, 3.0, gen)),
        "random normal": (torch.randn(B, H, N, D, generator=gen, device="cuda").half(),
                          torch.randn(B, H, N, D, generator=gen, device="cuda").half())}
for name, (q, k) in data.items():
    mass = sa.sageattn_tile_mass(q, k)
    rows = (N - 128 * torch.arange((N + 127) // 128, device="cuda")).clamp(max=128).float().view(1, 1, -1)
    emit()
    emit(f"### {name}")
    emit()
    emit("| cdfthreshd | density | recall mean | recall min over q-blocks |")
    emit("|---|---|---|---|")
    for cdf in (0.9, 0.95, 0.98):
        rec, kept = sa.plan_recall(sa.sparge_plan(q, k, simthreshd1=a.simthreshd1, cdfthreshd=cdf), mass)
        emit(f"| {cdf} | {float(kept.sum()) / mass.numel():.3f} | {float((rec * rows).sum() / (B * H * N)):.4f} | {float(rec.min()):.4f} |")
    emit()
    for rule in ("cdf", "topk"):
        t = sa.sparge_tune(q, k, target=0.95, rule=rule, simthreshd1=a.simthreshd1, steps=8, mass=mass)
        emit(f"- tuned {rule}: param {fmt(t.param, 4)}; met {t.met.tolist()}; recall {fmt(t.recall, 4)}; recall one grid step below "
             f"{fmt(t.recall_below, 4)}; density {fmt(t.density)}")
    del mass
write_out()
