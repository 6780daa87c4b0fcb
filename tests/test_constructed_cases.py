"""CPU proof that the bound of tests/constructed_cases.py is sound and has teeth.  Nothing here looks at a kernel.

Soundness: on every case the GPU test runs, the oracle's restatement of the kernel ("hip" flavour of attn_tile_loop: the
same roundings of P, the same row sums, fp32 accumulation) stays within ``bound`` of the fp64 reference.
Teeth: a float64 restatement of the loop that makes ONE deliberate mistake leaves the bound on the family meant to catch
that mistake.  Closed forms: the reference itself is checked against values known without computing a softmax."""
import math

import numpy as np
import pytest
import torch

import constructed_cases as C

_RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    if _RECORD:
        print("\noracle (hip flavour) on the constructed cases: largest |err| / bound   [o, lse2]")
        for (fam, pv, D), (ro, rl) in sorted(_RECORD.items()):
            print(f"  {fam:13s} {pv:5s} D={D:<4d} {ro:6.3f} {rl:6.3f}")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", C.PVS)
@pytest.mark.parametrize("family", C.FAMILIES)
def test_oracle_within_bound(family, pv, D):
    """ratio <= 1 for every element of every case; the scales of ramp / extreme_s / one_hot are uniform, so the
    granularity changes nothing the oracle sees there and one is enough."""
    grans = C.GRANS if family in ("scale_ladder", "coarse_lsb", "big_v") else ("per_warp",)
    worst = (0.0, 0.0)
    for label, c in C.family_cases(family, D, pv, grans):
        o, lse2 = C.oracle(c, pv)
        ro, rl = C.ratios(c, pv, o, lse2)
        assert ro <= 1.0 and rl <= 1.0, (label, ro, rl)
        worst = (max(worst[0], ro), max(worst[1], rl))
    _RECORD[(family, pv, D)] = worst


def _mutant_ratio(c, pv, mistake):
    o, lse2 = C.restate64(c, pv, mistake)
    return max(C.ratios(c, pv, o, lse2))


# (mistake, family that must catch it, builder).  head_dim 64 unless the mistake needs 128.
TEETH = [
    ("swap_key_groups", "scale_ladder", lambda: C.scale_ladder(64, 456, False, "per_thread")),
    ("tile3_scales_of_tile2", "scale_ladder", lambda: C.scale_ladder(64, 456, False, "per_thread")),
    ("tile3_scales_of_tile2", "scale_ladder", lambda: C.scale_ladder(64, 456, False, "per_warp")),
    ("tile3_scales_of_tile2", "scale_ladder", lambda: C.scale_ladder(128, 320, True, "per_block")),
    ("q_group_xor_1", "scale_ladder", lambda: C.scale_ladder(64, 456, False, "per_thread")),
    ("q_group_xor_1", "scale_ladder", lambda: C.scale_ladder(128, 456, False, "per_warp")),
    ("q_group_xor_1", "scale_ladder", lambda: C.scale_ladder(64, 456, False, "per_block")),
    ("drop_last_key", "one_hot", lambda: C.one_hot(64, 456, False, "per_warp", "last")),
    ("drop_last_key", "one_hot", lambda: C.one_hot(128, 456, False, "per_warp", "last", subnormal=True)),
    ("admit_key_N", "extreme_s", lambda: C.extreme_s(64, 456, False, "per_warp", "zero")),
    ("wrap_2_21", "extreme_s", lambda: C.extreme_s(128, 456, False, "per_warp", "corner")),
    ("clamp_p_2_5", "ramp", lambda: C.ramp(64, 456, False, "per_warp", "6", "ascending")),
    ("clamp_p_2_5", "ramp", lambda: C.ramp(128, 320, False, "per_warp", "6", "sawtooth")),
]


@pytest.mark.parametrize("i", range(len(TEETH)), ids=[f"{m}-{f}-{k}" for k, (m, f, _) in enumerate(TEETH)])
def test_bound_has_teeth(i):
    """each deliberate mistake exceeds the bound (ratio > 1) for every PV type it applies to"""
    mistake, family, build = TEETH[i]
    c = build()
    # P never exceeds 2^3 (times the offset) under FP8 PV: a clamp at 2^5 is no mistake there
    pvs = ("fp16", "bf16") if mistake == "clamp_p_2_5" else C.PVS
    for pv in pvs:
        clean = max(C.ratios(c, pv, *C.restate64(c, pv)))
        r = _mutant_ratio(c, pv, mistake)
        print(f"teeth: {mistake:22s} on {family:12s} {c['gran']:10s} D={c['D']:<3d} {pv:5s} ratio {r:12.1f}   (no mistake: {clean:.1e})")
        assert clean < 1e-3, (pv, clean)   # the restatement without the mistake IS the reference
        assert r > 1.0, (mistake, family, pv, r)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_zero_q_reference_is_the_mean(D, causal):
    c = C.extreme_s(D, 456, causal, "per_warp", "zero")
    for pv in C.PVS:
        ref = C.reference64(c, pv)
        V = C.v64(c, pv)
        if causal:
            n = torch.arange(1, 457, dtype=torch.float64)
            want, want_l = V.cumsum(2) / n.view(1, 1, -1, 1), torch.log2(n).view(1, 1, -1).expand(1, 2, -1)
        else:
            want, want_l = V.mean(2, keepdim=True).expand(1, 2, 150, D), torch.full((1, 2, 150), math.log2(456), dtype=torch.float64)
        assert (ref["o"] - want).abs().max() < 1e-13 and (ref["lse2"] - want_l).abs().max() < 1e-13


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("where", C.ONE_HOT_KEYS)
def test_one_hot_reference_is_the_v_row(D, where):
    """o = V[hot] to within 1 output ulp and lse2 = the hot logit (the 455 others together weigh 455 * 2^-78)"""
    for causal in (False, True):
        c = C.one_hot(D, 456, causal, "per_thread", where)
        hot = c["hot"]
        rows = slice(hot, None) if causal else slice(None)
        logit = (D * c["r"].double() * 127 * 2.0 ** -12).view(1, 1, -1)
        for pv in C.PVS:
            ref, V = C.reference64(c, pv), C.v64(c, pv)
            want = V[:, :, hot:hot + 1]
            assert ((ref["o"] - want).abs() <= C.out_ulp(want, pv))[:, :, rows].all()
            assert (ref["lse2"] - logit)[:, :, rows].abs().max() < 1e-12


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("shape", C.RAMP_SHAPES)
def test_ramp_is_rank_one_and_hits_its_steps_exactly(D, shape):
    for step, units in C.RAMP_UNITS.items():
        c = C.ramp(D, 512, False, "per_thread", step, shape)
        S = (c["q8"].to(torch.int64) @ c["k8"].to(torch.int64).transpose(2, 3))  # exact integers
        assert torch.equal(S[0, 0], c["r"].to(torch.int64).view(-1, 1) * c["K"].view(1, -1))
        assert S.abs().max() < 2 ** 22
        # fp32, associated as the kernel does: (q_scale * logit_mult) * k_scale, times float(S)
        sc = (c["q_scale_rows"] * torch.tensor(c["logit_mult"])).unsqueeze(-1) * c["k_scale_cols"].unsqueeze(2)
        t = S.float() * sc
        assert t.dtype == torch.float32 and torch.equal(t.double(), S.double() * 2.0 ** -12)
        steep = t[0, 0, 0].view(8, 64).amax(-1)              # row 0 has r = 4: the steepest trend
        assert c["r"][0] == 4
        levels = torch.tensor(C._ramp_levels(shape, 8), dtype=torch.float32)
        want = torch.tensor(np.float32(units) / np.float32(1024))  # 0.5, thr - 2^-10, thr, thr + 2^-10, 40: exact in fp32
        assert float(want) * 1024 == units
        d_t, d_l = steep[1:] - steep[:-1], levels[1:] - levels[:-1]  # fp32 subtraction, exact
        assert torch.equal(d_t, d_l * want)
        # every 32-row wave holds every trend, both signs
        for w0 in range(0, 150 - 31, 32):
            assert set(c["r"][w0:w0 + 32].tolist()) == {4, -4, 2, -2, 1, -1, 0}


def test_extreme_scores_are_the_corners():
    c = C.extreme_s(128, 456, False, "per_warp", "corner")
    S = C.scores(c)
    assert S.max() == 2 ** 21 and S.min() == -2080768
    assert torch.equal(S[0, 0, 0, :64].unique(), torch.tensor([-2080768.0, 2097152.0], dtype=torch.float64))
    assert abs(float((S.max() - S.min()) * C.scale_matrix(c).max()) - 15.94) < 0.01
    c = C.extreme_s(64, 456, False, "per_warp", "corner")
    assert C.scores(c).max() == 2 ** 20 and C.scores(c).min() == -1040384


def test_coarse_lsb_and_delta():
    """the row LSB is what the family says, and delta is 0.75 s for small scores, 0.875 s at S = 2^21"""
    for e in (-6, -5, -4):
        assert float(C.row_lsb(C.coarse_lsb(64, 456, False, "per_thread", e)).max()) == 2.0 ** e
    assert float(C.row_lsb(C.scale_ladder(64, 456, False, "per_thread")).max()) == 2.0 ** -12
    assert (C.BIAS + 2 ** 21) * 2.0 ** -24 == 0.875 and C.BIAS * 2.0 ** -24 == 0.75


def test_logit_mult_is_a_power_of_two_in_fp32():
    assert np.float32(C.SM_SCALE) * np.float32(1.4426950408889634) == np.float32(0.125) == np.float32(C.LOGIT_MULT)


# ---- subsets of the keys: block maps, key lengths, split-KV ------------------------------------------------------------

_SUB = {}


@pytest.fixture(scope="module", autouse=True)
def _sub_table():
    yield
    if _SUB:
        print("\noracle (hip flavour) on the SUBCASES: largest |err| / bound   [o, lse2]")
        for (what, fam, pv, D), (ro, rl) in sorted(_SUB.items()):
            print(f"  {what:10s} {fam:13s} {pv:5s} D={D:<4d} {ro:6.3f} {rl:6.3f}")


def _sub_record(what, fam, pv, D, ro, rl):
    a, b = _SUB.get((what, fam, pv, D), (0.0, 0.0))
    _SUB[(what, fam, pv, D)] = (max(a, ro), max(b, rl))


def _oracle32(c, pv):
    """the oracle's partial result as the split-KV workspace holds it: not rounded to an output type"""
    return C.O.attn_tile_loop(c["q8"], c["k8"], C.v_of(c, pv), c["q_scale_rows"], c["k_scale_cols"], logit_mult=c["logit_mult"],
                              is_causal=c["causal"], pv="fp8" if pv == "fp8" else "fp16",
                              v_scale=c["v_scale"] if pv == "fp8" else None, out_dtype=torch.float32, flavor="hip")


def _tile_lists():
    seen = []
    for m in C.SUBSET_MAPS.values():
        for per_head in m:
            for tiles in per_head:
                if tiles not in seen:
                    seen.append(tiles)
    return seen


def test_subcase_is_the_case_on_the_gathered_keys():
    """subcase against a reference computed the long way: the full case with the unlisted keys masked out"""
    c = C.scale_ladder(64, 456, False, "per_thread")
    for tiles, length in (([0, 2, 4, 6], None), ([7], None), ([1, 3, 5, 7], 257), (None, 257), (None, 1)):
        d = C.subcase(c, tiles, length)
        n = torch.arange(456)
        keep = (n < (456 if length is None else length))
        if tiles is not None:
            keep &= torch.isin(n // 64, torch.tensor(tiles))
        assert d["N"] == int(keep.sum()) and d["v_f8t"].shape[-1] % 64 == 0
        for pv in C.PVS:
            t = (C.scores(c) * C.scale_matrix(c)).masked_fill(~keep.view(1, 1, 1, -1), float("-inf"))
            W = torch.softmax(t * math.log(2), dim=-1)
            ref = C.reference64(d, pv)
            assert (W @ C.v64(c, pv) - ref["o"]).abs().max() < 1e-12
            assert (torch.logsumexp(t * math.log(2), -1) / math.log(2) - ref["lse2"]).abs().max() < 1e-11
    cc = C.subcase(C.scale_ladder(64, 456, True, "per_warp"), length=257)
    assert cc["causal"] and cc["M"] == 456 and cc["N"] == 257
    with pytest.raises(AssertionError):
        C.subcase(C.scale_ladder(64, 456, True, "per_warp"), [1, 2])


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", C.PVS)
@pytest.mark.parametrize("family", C.SUBSET_FAMILIES)
def test_oracle_within_bound_on_map_and_length_subcases(family, pv, D):
    """every subcase tests/test_constructed_subsets_gpu.py checks a kernel against: each tile list of SUBSET_MAPS, each key
    length (causal and not), and the lists clipped to the lengths"""
    grans = ("per_warp", "per_thread") if family == "scale_ladder" else ("per_warp",)
    for causal in (False, True):
        for label, c in C.subset_cases(family, D, pv, grans, causal):
            subs = [("length", None, n) for n in C.KVLEN_LENGTHS]
            if not causal:
                subs += [("map", t, None) for t in _tile_lists()]
                subs += [("map+length", [x for x in t if 64 * x < n], n) for t in _tile_lists() for n in C.KVLEN_LENGTHS[1:]]
            for what, tiles, n in subs:
                if tiles is not None and not tiles:
                    continue  # a q-block without a tile below the length: o = 0, lse = -inf, no softmax
                d = C.subcase(c, tiles, n)
                ro, rl = C.ratios(d, pv, *C.oracle(d, pv))
                _sub_record(what, family, pv, D, ro, rl)
                assert ro <= 1.0 and rl <= 1.0, (label, what, tiles, n, ro, rl)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("gran", ["per_warp", "per_thread"])
def test_anchored_cases_come_back_from_the_quantizers(gran, D):
    """Q = q8 * 2^e of every anchored case the GPU test uses, through the oracle's Q quantizers (per_warp: the CUDA numerics;
    per_thread: the Triton numerics, scale + 1e-7): q8 and the scales 2^e exactly, in fp16 and in bf16; and every scale
    product of the case is still a power of two"""
    quant = C.O.per_warp_int8 if gran == "per_warp" else C.O.per_thread_int8
    for family in C.SPLIT_FAMILIES:
        for N, _ in C.SPLIT_CONFIGS:
            for label, c in C.split_cases(family, D, N, gran):
                assert float(c["q_scale"].min()) >= 2.0
                sc = C.scale_matrix(c)
                assert torch.equal(torch.log2(sc), torch.log2(sc).round()), label
                for dt in (torch.float16, torch.bfloat16):
                    q8, qs, _, _ = quant(C.q_real(c, dt), torch.zeros(1, 1, 64, D, dtype=dt))
                    assert torch.equal(q8, c["q8"]), (label, dt)
                    assert torch.equal(C.O.expand_q_scale(qs, c["M"], gran), c["q_scale_rows"]), (label, dt)
    c0 = C.ramp(D, 512, False, gran, "40", anchor=True)
    q0 = (c0["q8"].float() * 1.0).half()  # e = 0: the per-thread scale comes back as 1.0000001
    _, qs, _, _ = C.O.per_thread_int8(q0, torch.zeros(1, 1, 64, D).half())
    assert float(qs[0, 0, 0]) == float(np.float32(1.0000001)) != 1.0


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", C.PVS)
@pytest.mark.parametrize("family", C.SPLIT_FAMILIES)
def test_oracle_partials_and_fp32_merge_within_merged_bound(family, pv, D):
    """every split configuration the GPU test runs: the oracle's fp32 partial of each split inside ``bound`` (no output
    ulps) of its subcase, and the merge kernel's arithmetic in numpy float32 over those partials, rounded once to fp16 and
    to bf16, inside ``merged_bound`` -- o, the raw lse2 and the finished LSE with a non-zero q.km"""
    km = C.split_km(D, True)
    for N, splits in C.SPLIT_CONFIGS:
        for label, c in C.split_cases(family, D, N, "per_warp"):
            qkm_full = C.split_qkm(c, km)
            for n in C.SPLIT_LENGTHS[:2]:
                cn = c if n is None else C.subcase(c, length=n)
                ref = C.reference64(cn, pv)
                parts = {}
                for S in splits:
                    subs = C.split_subcases(cn, S)
                    os_, ls = [], []
                    for d in subs:
                        if d["tiles"] not in parts:
                            parts[d["tiles"]] = _oracle32(d, pv)
                            o_b, l_b = C.bound(d, pv, out_ulps=0)
                            r = C.reference64(d, pv)
                            ro = float(((parts[d["tiles"]][0].double() - r["o"]).abs() / o_b).max())
                            rl = float(((parts[d["tiles"]][1].double() - r["lse2"]).abs() / l_b).max())
                            _sub_record("partial", family, pv, D, ro, rl)
                            assert ro <= 1.0 and rl <= 1.0, (label, n, S, d["tiles"], ro, rl)
                        os_.append(parts[d["tiles"]][0])
                        ls.append(parts[d["tiles"]][1])
                    o32, l32 = C.merge_fp32(torch.stack(os_), torch.stack(ls))
                    lse = torch.from_numpy((l32.numpy() / np.float32(1.44269504)
                                            + (qkm_full.numpy() / c["sm_scale"]).astype(np.float32) * np.float32(c["sm_scale"])).astype(np.float32))
                    for dt in (torch.float16, torch.bfloat16):
                        ro, rl = C.merged_ratios(cn, pv, S, o32.to(dt), lse, qkm_full, dt)
                        _sub_record("merged", family, pv, D, ro, rl)
                        assert ro <= 1.0 and rl <= 1.0, (label, n, S, dt, ro, rl)
                    l2_b = C.merged_bound(cn, pv, S)[1]
                    assert ((l32.double() - ref["lse2"]).abs() <= l2_b).all(), (label, n, S)


def test_split_ramps_cover_the_regimes_of_the_merge():
    """from the fp64 reference alone: over the step-40 ramps (ascending, descending, sawtooth, peak) and the split counts run at
    N = 512, the largest LSE gap between two non-empty splits of a row lies below 1, in 1..24, in 24..126, in the window
    126..149 where fp32 weights are subnormal, and above 150; the dominant split is the first, a middle one and the last"""
    seen, dominant = set(), set()
    for label, c in C.split_cases("ramp", 64, 512, "per_warp"):
        for S in C.SPLIT_CONFIGS[0][1]:
            g = C.split_gaps(c, "fp16", S)
            for name, lo, hi in (("<1", -1, 1), ("1..24", 1, 24), ("24..126", 24, 126), ("126..149", 126, 149), (">150", 150, 1e9)):
                if bool(((g > lo) & (g < hi)).any()):
                    seen.add(name)
            l = torch.stack([C.reference64(d, "fp16")["lse2"] for d in C.split_subcases(c, S)])
            arg = l.argmax(0)[g > 150]
            dominant |= {"first" if a == 0 else "last" if a == l.shape[0] - 1 else "middle" for a in arg.tolist()}
    assert seen == {"<1", "1..24", "24..126", "126..149", ">150"}, seen
    assert dominant == {"first", "middle", "last"}, dominant


def test_offset_case_has_large_lses_small_gaps_and_a_small_delta():
    for D in (64, 128):
        c = C.offset(D, 512, "per_warp")
        smax = float(C.scores(c).abs().max())
        delta = (C.BIAS + smax) * 2.0 ** -24 * 2.0 ** -7 + 2.0 ** -24 * (smax * 2.0 ** -7 + C.FP8_OFFSET)
        assert float(C.row_lsb(c).max()) == 2.0 ** -7 and delta < 2.0 ** -6
        for S in C.SPLIT_CONFIGS[0][1]:
            l = torch.stack([C.reference64(d, "fp16")["lse2"] for d in C.split_subcases(c, S)])
            assert float(l.abs().min()) >= 2.0 ** 10 and float(C.split_gaps(c, "fp16", S).max()) < 1.0, S


def test_zero_q_merged_reference_weighs_a_split_by_its_key_count():
    c = C.anchor(C.extreme_s(64, 456, False, "per_warp", "zero"))
    subs = C.split_subcases(c, 3)
    l = torch.stack([C.reference64(d, "fp16")["lse2"] for d in subs])
    assert [d["N"] for d in subs] == [192, 192, 72]
    assert (torch.exp2(l - C.reference64(c, "fp16")["lse2"])[:, 0, 0, 0] - torch.tensor([192, 192, 72]).double() / 456).abs().max() < 1e-14


_KM64 = lambda: C.split_km(64, True)
# (mistake, family that must catch it, case builder, S, length, tiles)
SPLIT_TEETH = [
    ("split_scales_from_tile0", "scale_ladder", lambda: C.anchor(C.scale_ladder(64, 512, False, "per_warp")), 3, None),
    ("split_scales_from_tile0", "scale_ladder", lambda: C.anchor(C.scale_ladder(128, 456, False, "per_thread")), 7, None),
    ("split_tail_unmasked", "extreme_s", lambda: C.anchor(C.extreme_s(64, 456, False, "per_warp", "zero")), 3, None),
    ("split_tail_unmasked", "extreme_s", lambda: C.anchor(C.extreme_s(64, 512, False, "per_warp", "zero")), 2, 257),
    ("merge_equal_weights", "ramp", lambda: C.ramp(64, 512, False, "per_warp", "40", "ascending", anchor=True), 4, None),
    ("merge_base_e_weights", "ramp", lambda: C.ramp(64, 512, False, "per_warp", "0.5", "ascending", anchor=True), 4, None),
    ("merge_drops_last_split", "ramp", lambda: C.ramp(64, 512, False, "per_warp", "40", "ascending", anchor=True), 5, None),
    ("correction_added_per_split", "ramp", lambda: C.ramp(64, 512, False, "per_warp", "40", "descending", anchor=True), 2, None),
    ("correction_added_per_split", "scale_ladder", lambda: C.anchor(C.scale_ladder(128, 456, False, "per_thread")), 7, None),
    ("length_rounded_up_to_tile", "extreme_s", lambda: C.anchor(C.extreme_s(64, 512, False, "per_warp", "zero")), 3, 257),
    ("length_rounded_up_to_tile", "one_hot", lambda: C.anchor(C.one_hot(64, 512, False, "per_warp", 257)), 3, 257),
]


@pytest.mark.parametrize("i", range(len(SPLIT_TEETH)), ids=[f"{m}-{f}-{k}" for k, (m, f, *_) in enumerate(SPLIT_TEETH)])
def test_merged_bound_has_teeth(i):
    """each deliberate mistake of the split-KV restatement leaves merged_bound (ratio > 1); without it the restatement IS
    the reference (< 1e-3)"""
    mistake, family, build, S, n = SPLIT_TEETH[i]
    c = build()
    cn = c if n is None else C.subcase(c, length=n)
    qkm = C.split_qkm(c, C.split_km(c["D"], True))
    assert float(qkm.abs().max()) > 0.1
    for pv in C.PVS:
        o, _, lse = C.restate_split64(c, pv, S, n, None, qkm)
        clean = max(C.merged_ratios(cn, pv, S, o, lse, qkm))
        o, _, lse = C.restate_split64(c, pv, S, n, mistake, qkm)
        r = max(C.merged_ratios(cn, pv, S, o, lse, qkm))
        print(f"teeth: {mistake:28s} on {family:12s} D={c['D']:<3d} S={S:<2d} {pv:5s} ratio {r:12.1f}   (no mistake: {clean:.1e})")
        assert clean < 1e-3, (pv, clean)
        assert r > 1.0, (mistake, family, pv, r)


SUBSET_TEETH = [
    ("list_position_for_tile_index", "scale_ladder", lambda: C.scale_ladder(64, 456, False, "per_warp"), [1, 3, 5, 7], None),
    ("list_position_for_tile_index", "scale_ladder", lambda: C.scale_ladder(128, 456, False, "per_thread"), [3], None),
    ("length_rounded_up_to_tile", "extreme_s", lambda: C.extreme_s(64, 456, False, "per_warp", "zero"), None, 257),
    ("length_rounded_up_to_tile", "one_hot", lambda: C.one_hot(64, 456, True, "per_warp", 257), None, 257),
    ("length_rounded_up_to_tile", "one_hot", lambda: C.one_hot(64, 456, False, "per_warp", 257), [0, 2, 4], 257),
]


@pytest.mark.parametrize("i", range(len(SUBSET_TEETH)), ids=[f"{m}-{f}-{k}" for k, (m, f, *_) in enumerate(SUBSET_TEETH)])
def test_subcase_bound_has_teeth(i):
    mistake, family, build, tiles, n = SUBSET_TEETH[i]
    c = build()
    d = C.subcase(c, tiles, n)
    for pv in C.PVS:
        clean = max(C.ratios(d, pv, *C.restate_subset64(c, pv, tiles, n)))
        r = max(C.ratios(d, pv, *C.restate_subset64(c, pv, tiles, n, mistake)))
        print(f"teeth: {mistake:28s} on {family:12s} D={c['D']:<3d} {pv:5s} ratio {r:12.1f}   (no mistake: {clean:.1e})")
        assert clean < 1e-3, (pv, clean)
        assert r > 1.0, (mistake, family, pv, r)


# ---- attn_mask: structured masks as part of a case ----------------------------------------------------------------------

_MASK = {}
_MASK_DTYPE = {"fp16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture(scope="module", autouse=True)
def _mask_table():
    yield
    if _MASK:
        print("\noracle (hip flavour, attn_mask) on the masked cases: largest |err| / bound   [o, lse2]")
        for (name, fam, pv, D), (ro, rl) in sorted(_MASK.items()):
            print(f"  {name:15s} {fam:13s} {pv:5s} D={D:<4d} {ro:6.3f} {rl:6.3f}")


def _small_masked(c, pv, M, N):
    """the case cut to (M, N) under each pattern of SMALL_PATTERNS at that size"""
    d = C.cut_case(c, M, N)
    for name, mask in C.mask_patterns(M, N, _MASK_DTYPE[pv], names=C.SMALL_PATTERNS):
        yield name, C.with_mask(d, mask)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", ["fp16", "bf16"])
@pytest.mark.parametrize("family", C.SUBSET_FAMILIES)
def test_oracle_within_bound_under_masks(family, pv, D):
    """every masked case tests/test_constructed_masks_gpu.py checks the kernel against: the oracle called with attn_mask stays
    within the bound on every element of every row that keeps a key, under every pattern at N = 456 and under the two small
    patterns at MASK_SMALL_SHAPES.  Only row_switch has rows without a key, ceil((M - 5) / 16) per slice."""
    masks = dict(C.mask_patterns(dtype=_MASK_DTYPE[pv]))
    for label, c in C.subset_cases(family, D, pv, grans=C.GRANS):
        todo = [(name, C.with_mask(c, mask, name)) for name, mask in masks.items()]
        if label.endswith(C.GRANS[0]):
            todo += [(f"{name}", d) for M, N in C.MASK_SMALL_SHAPES for name, d in _small_masked(c, pv, M, N)]
        for name, d in todo:
            dead = C.no_key_rows(d)
            want = -(-(d["M"] - 5) // 16) if name == "row_switch" else 0
            assert bool((dead.sum(-1) == want).all()), (label, name)
            ro, rl = C.mask_ratios(d, pv, *C.oracle(d, pv))
            a, b = _MASK.get((name, family, pv, D), (0.0, 0.0))
            _MASK[(name, family, pv, D)] = (max(a, ro), max(b, rl))
            assert ro <= 1.0 and rl <= 1.0, (label, name, d["M"], d["N"], ro, rl)


def test_mask_patterns_are_what_they_say():
    """structure of the patterns at M = 150, N = 456: no two (batch, head) slices of a key-dependent pattern are equal; waves of
    one q-block skip different tiles and some wave has tile 0 off; the lone row; first keys beyond tile 0; the broadcast
    patterns are expanded views; the additive values are exact in fp16 and in bf16"""
    for name, m in C.mask_patterns():
        assert tuple(m.shape) == (2, 2, 150, 456), name
        sl = [m[b, h] for b in range(2) for h in range(2)]
        if name not in ("row_switch", "key_padding"):
            assert all(not torch.equal(sl[i], sl[j]) for i in range(4) for j in range(i)), name
        if m.dtype != torch.bool:
            if name not in ("pad_1e4", "rows_1e4"):  # (-1e4 is -9984 in bf16)
                assert torch.equal(C.mask_pattern(name, dtype=torch.bfloat16).double(), m.double()), name
    assert not torch.equal(*C.mask_pattern("key_padding")[:, 0])
    assert C.mask_pattern("key_padding").stride()[1:3] == (0, 0) and C.mask_pattern("row_switch").stride(3) == 0
    assert C.mask_pattern("row_const").stride(3) == 0
    assert float(C.mask_pattern("pad_1e4", dtype=torch.bfloat16)[0, 0, 0, 300]) == -9984.0
    wts = C.mask_pattern("wave_tile_skip")
    tiles = torch.stack([wts[:, :, 32 * g:32 * g + 32, 64 * j:64 * j + 64].flatten(2).any(-1) for g in range(5)
                         for j in range(8)], -1).view(2, 2, 5, 8)                # [b,h,wave,tile]: does the wave compute the tile
    for b in range(2):
        for h in range(2):
            s = 3 * b + h
            assert torch.equal(tiles[b, h], (torch.arange(5).view(5, 1) + torch.arange(8).view(1, 8) + s) % 3 != 0)
            assert not torch.equal(tiles[b, h, 0], tiles[b, h, 1]) and not tiles[b, h, :, 0].all()
            j = C.lone_row_tile(s)
            blk = wts[b, h, 0:32, 64 * j:64 * j + 64]
            assert not blk[:31].any() and blk[31].any()
            assert wts[b, h, :31].any(-1).all()                                # the switched-off rows keep keys elsewhere
    first = C.mask_pattern("late_first_key").float().argmax(-1)
    assert torch.equal(first[0, 0], (37 * torch.arange(150)) % 456)
    for g in range(5):
        assert len(set((first[0, 0, 32 * g:32 * g + 32] // 64).tolist())) >= 4  # the rows of a wave start in different tiles
    assert float((first >= 64).double().mean()) > 0.8
    ro = C.mask_pattern("ragged_only")
    assert ro[:, :, 32:64, :448].sum() == 0 and bool(ro[:, :, 32:64, 452:].all()) and bool(ro[:, :, :32].all())
    assert bool(C.mask_pattern("single_key").sum(-1).eq(1).all())
    ni = C.mask_pattern("neg_inf")
    assert bool(torch.isinf(ni[:, :, :, :64]).all()) and bool((~torch.isinf(ni)).any(-1).all())


@pytest.mark.parametrize("D", [64, 128])
def test_masked_reference_identities(D):
    """three closed forms of the masked fp64 reference.  single_key: o is the V row of the row's key and lse2 its logit.
    key_padding: batch slice b equals the reference of the first 257 - 3 b keys (cached_subcase).  row_const: the unmasked o,
    lse2 shifted by the row's constant."""
    c = C.scale_ladder(D, C.SUBSET_N, False, "per_thread")
    t = C.scores(c) * C.scale_matrix(c)
    b, h, r, n, s = C._mask_index(c["M"], c["N"], 2)
    for pv in ("fp16", "bf16"):
        plain, V = C.reference64(c, pv), C.v64(c, pv)
        d = C.with_mask(c, C.mask_pattern("single_key"))
        ref = C.reference64(d, pv)
        key = ((61 * r + s) % c["N"]).expand(2, 2, c["M"], 1)
        assert torch.equal(ref["o"], torch.gather(V.expand(2, -1, -1, -1), 2, key.expand(-1, -1, -1, D)))
        assert torch.equal(ref["lse2"], torch.gather(t.expand(2, -1, -1, -1), 3, key).squeeze(-1))
        d = C.with_mask(c, C.mask_pattern("key_padding"))
        ref = C.reference64(d, pv)
        for bb in range(2):
            sub = C.reference64(C.cached_subcase(c, length=C.KEY_PAD_LEN - 3 * bb), pv)
            assert (ref["o"][bb:bb + 1] - sub["o"]).abs().max() < 1e-13 and (ref["lse2"][bb:bb + 1] - sub["lse2"]).abs().max() < 1e-11
            assert (ref["sumabsv"][bb:bb + 1] / sub["sumabsv"] - 1).abs().max() < 1e-13
        d = C.with_mask(c, C.mask_pattern("row_const", dtype=_MASK_DTYPE[pv]))
        ref = C.reference64(d, pv)
        const = (3 * ((r + s) % 11) - 15).double().expand(2, 2, c["M"], 1).squeeze(-1)
        assert (ref["o"] - plain["o"]).abs().max() < 1e-13 and (ref["lse2"] - (plain["lse2"] + const)).abs().max() < 1e-11
        assert const.abs().max() == 15 and not torch.equal(const[0, 0], const[1, 1])


_SL = lambda D=64, gran="per_thread": C.scale_ladder(D, C.SUBSET_N, False, gran)
# (mistake, family that must catch it, pattern, case builder, (M, N) or None for 150 x 456)
MASK_TEETH = [
    ("mask_next_row", "scale_ladder", "late_first_key", _SL, None),
    ("mask_next_row", "ramp", "rows_1e4", lambda: C.ramp(64, 456, False, "per_warp", "40", "sawtooth"), None),
    ("mask_next_key", "scale_ladder", "first_tile_off", _SL, None),
    ("mask_next_key", "one_hot", "neg_inf", lambda: C.one_hot(64, 456, False, "per_warp", 200), None),
    ("mask_head_zero", "scale_ladder", "wave_tile_skip", _SL, None),
    ("mask_head_zero", "extreme_s", "row_const", lambda: C.extreme_s(64, 456, False, "per_warp", "zero"), None),
    ("mask_batch_zero", "scale_ladder", "key_padding", _SL, None),
    ("mask_batch_zero", "scale_ladder", "grid", lambda: _SL(128, "per_warp"), None),
    ("skip_by_first_row", "scale_ladder", "wave_tile_skip", _SL, None),
    ("skip_by_first_row", "one_hot", "late_first_key", lambda: C.one_hot(64, 456, False, "per_warp", 200), None),
    ("tail_run_unread", "scale_ladder", "late_first_key", _SL, (33, 65)),
    ("tail_run_unread", "scale_ladder", "neg_inf", _SL, (5, 3)),
    ("run_reversed", "scale_ladder", "single_key", _SL, None),
    ("run_reversed", "extreme_s", "pad_1e4", lambda: C.extreme_s(64, 456, False, "per_warp", "zero"), None),
    ("additive_times_scale", "scale_ladder", "grid", _SL, None),
    ("additive_in_nats", "ramp", "row_const", lambda: C.ramp(64, 456, False, "per_warp", "6", "ascending"), None),
    ("additive_in_nats", "scale_ladder", "neg_inf", _SL, None),
    ("bf16_read_as_fp16", "scale_ladder", "grid", _SL, None),
    ("bf16_read_as_fp16", "one_hot", "pad_1e4", lambda: C.one_hot(64, 456, False, "per_warp", 200), None),
]


def test_every_mask_mistake_has_a_tooth():
    assert {m for m, *_ in MASK_TEETH} == set(C.MASK_MISTAKES)


@pytest.mark.parametrize("i", range(len(MASK_TEETH)), ids=[f"{m}-{f}-{p}" for m, f, p, *_ in MASK_TEETH])
def test_mask_bound_has_teeth(i):
    """each deliberate mistake of the attn_mask restatement leaves the bound (ratio > 1) on the named (family, pattern);
    without it the restatement IS the reference (< 1e-3)"""
    mistake, family, pattern, build, shape = MASK_TEETH[i]
    c = build()
    if shape is not None:
        c = C.cut_case(c, *shape)
    additive = pattern in C.ADD_PATTERNS
    for pv in ("fp16", "bf16"):
        if mistake == "bf16_read_as_fp16" and pv != "bf16":
            continue
        d = C.with_mask(c, C.mask_pattern(pattern, c["M"], c["N"], _MASK_DTYPE[pv]))
        assert (d["mask"].dtype != torch.bool) == additive
        clean = max(C.mask_ratios(d, pv, *C.restate_mask64(d, pv)))
        r = max(C.mask_ratios(d, pv, *C.restate_mask64(d, pv, mistake)))
        print(f"teeth: {mistake:22s} on {family:12s} {pattern:15s} D={c['D']:<3d} {pv:5s} ratio {r:12.1f}   (no mistake: {clean:.1e})")
        assert clean < 1e-3, (pv, clean)
        assert r > 1.0, (mistake, family, pattern, pv, r)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("backend", list(C.PUBLIC_BACKENDS))
def test_public_forms_come_back_from_the_quantizers(backend, D):
    """Q and K of every public_form case, through the oracle's quantizers of the backend ("triton": per-thread, scale + 1e-7;
    "cuda": per-block with sm_scale * log2e folded into Q, the CUDA rounding) without K smoothing: q8, k8 and both compact
    scales come back exactly, in fp16 and in bf16, and the oracle with a mask stays inside the bound on the form"""
    for label, d in C.public_cases(D, backend):
        sc = C.scale_matrix(d)
        assert torch.equal(torch.log2(sc), torch.log2(sc).round()), label
        assert float(d["q_real_rows"].min()) >= 2.0 and float(d["k_scale"].min()) >= 2.0
        for dt in (torch.float16, torch.bfloat16):
            q, k = C.public_qk(d, dt)
            if backend == "triton":
                q8, qs, k8, ks = C.O.per_thread_int8(q, k)
            else:
                q8, qs, k8, ks = C.O.per_block_int8(q, k, sm_scale=d["sm_scale"], rounding="cuda")
            assert torch.equal(q8, d["q8"]) and torch.equal(k8, d["k8"]), (label, dt)
            gran = C.PUBLIC_BACKENDS[backend]  # (the groups of rows >= M hold no row: compare the scales row by row)
            assert torch.equal(C.O.expand_q_scale(qs, d["M"], gran), d["q_scale_rows"]), (label, dt)
            assert torch.equal(C.O.expand_k_scale(ks, d["N"], gran), d["k_scale_cols"]), (label, dt)
        for pv in ("fp16", "bf16"):
            for name, mask in C.mask_patterns(dtype=_MASK_DTYPE[pv], names=C.PUBLIC_PATTERNS):
                m = C.with_mask(d, mask)
                ro, rl = C.mask_ratios(m, pv, *C.oracle(m, pv))
                assert ro <= 1.0 and rl <= 1.0, (label, name, pv, ro, rl)


# ---- layouts: stacked, packed and tile-major calls (tests/test_constructed_layouts_gpu.py) ----------------------------------

LAYOUT_SHAPES = ((64, "per_thread"), (128, "per_warp"), (64, "per_block"))  # (head_dim, granularity) of the CPU proofs
_SAME = ("q8", "k8", "q_scale", "k_scale", "q_scale_rows", "k_scale_cols", "v_f16", "v_bf16")


def _bytes(t):
    return t.view(torch.uint8) if t.dtype == torch.float8_e4m3fn else t


@pytest.mark.parametrize("gran", C.GRANS)
def test_layout_builders_hold_each_case_where_a_kernel_reads_it(gran):
    """read_stack / read_pack / read_tiles without a mistake return the operands of the slot's own case bit for bit, so a slice
    of a call's result IS that case's result; the poison of the tile-major buffers and the NaN scale slots of a pack are where
    the docstrings say"""
    for causal in (False, True):
        st = C.stack_slots(64, 456, causal, gran)
        assert tuple(st["q8"].shape) == (2, 4, st["M"], 64) and tuple(st["k8"].shape) == (2, 2, 456, 64)
        assert tuple(st["v_scale"].shape) == (2, 2, 64) and st["q_scale"].shape[:2] == (2, 4) and st["k_scale"].shape[:2] == (2, 2)
        tm = C.tile_major(st)
        for b in range(2):
            for hk in range(2):
                own = st["grid"][b][hk]
                for d in (C.read_stack(st, b, hk), C.read_tiles(tm, b, hk)):
                    assert all(torch.equal(_bytes(d[k]), _bytes(own[k])) for k in _SAME + ("v_f8t", "v_scale")), (b, hk)
        kt, T = tm["layout"]("fp16")[0], tm["T"]
        assert kt > 2 * 2 * 64 * 64 and all(x > 0 for x in tm["layout"]("fp8")) and all(x % 4 == 0 for x in tm["layout"]("fp8")[2:])
        assert bool((tm["k8"][:, :, :, 64:] == 127).all()) and bool((tm["k8"][T - 1, :, :, 8:] == 127).all())  # 456 = 7 * 64 + 8
        assert bool(torch.isnan(tm["v_f16"][:, :, :, 64:]).all()) and bool(torch.isnan(tm["v_bf16"][T - 1, :, :, 8:]).all())
        assert bool((tm["v_f8t"].view(torch.uint8)[..., 64:] == 0x7F).all()) and bool(torch.isnan(tm["k_scale"][..., tm["per_tile"]:]).all())
        pk = C.pack_cases(64, gran, causal)
        assert pk["Ms"] == [m for m, _ in (C.PACK_CUTS_CAUSAL if causal else C.PACK_CUTS)]
        assert pk["Ns"] == [n for _, n in (C.PACK_CUTS_CAUSAL if causal else C.PACK_CUTS)]
        assert tuple(pk["q8"].shape) == (sum(pk["Ms"]), 4, 64) and tuple(pk["k8"].shape) == (sum(pk["Ns"]), 2, 64)
        assert tuple(pk["q_scale"].shape) == (pk["S"], 4, pk["gq"]) and tuple(pk["k_scale"].shape) == (pk["S"], 2, pk["gk"])
        used = 0
        for s, row in enumerate(pk["cases"]):
            for hk, own in enumerate(row):
                used += own["q_scale"].numel() + own["k_scale"].numel()
                if own["N"]:
                    d = C.read_pack(pk, s, hk)
                    assert all(torch.equal(d[k], own[k]) for k in _SAME), (s, hk)
        finite = int(torch.isfinite(pk["q_scale"]).sum() + torch.isfinite(pk["k_scale"]).sum())
        assert finite == used and pk["q_scale"].numel() + pk["k_scale"].numel() > used


@pytest.mark.parametrize("D,gran", LAYOUT_SHAPES)
def test_layout_slices_are_sound(D, gran):
    """the oracle's restatement of the kernel on every slice of the stacked calls (dense and causal), on every sequence of the
    packed calls and on the causal (M, N) cuts stays within ``bound`` of the slice's own case, every element"""
    worst = {}
    for causal in (False, True):
        st = C.stack_slots(D, 456, causal, gran)
        for pv in C.PVS:
            for b in range(2):
                for hk in range(2):
                    r = C.ratios(st["grid"][b][hk], pv, *C.oracle(C.read_stack(st, b, hk), pv))
                    worst["stack"] = max(worst.get("stack", 0.0), *r)
                    assert max(r) <= 1.0, ("stack", causal, pv, b, hk, r)
        pk = C.pack_cases(D, gran, causal)
        for pv in ("fp16", "bf16"):
            for s, row in enumerate(pk["cases"]):
                for hk, own in enumerate(row):
                    if own["N"]:
                        r = C.ratios(own, pv, *C.oracle(C.read_pack(pk, s, hk), pv))
                        worst["pack"] = max(worst.get("pack", 0.0), *r)
                        assert max(r) <= 1.0, ("pack", causal, pv, s, hk, r)
    for label, c in C.causal_cut_cases(D, gran):
        for pv in C.PVS:
            r = C.ratios(c, pv, *C.oracle(c, pv))
            worst["cut"] = max(worst.get("cut", 0.0), *r)
            assert max(r) <= 1.0, (label, pv, r)
            assert max(C.ratios(c, pv, *C.restate_causal64(c, pv))) < 1e-3  # top-left IS the reference at M != N
    print(f"layout soundness D={D} {gran}: largest oracle ratio " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


def _layout_mutants(mistake, D, gran, pv):
    """yield (slice label, ratio without the mistake, ratio with it) over the slices the mistake should corrupt"""
    both = lambda own, f: (max(C.ratios(own, pv, *f(None))), max(C.ratios(own, pv, *f(mistake))))
    if mistake == "head_scales_of_kv_head_0":
        st = C.stack_slots(D, 456, False, gran)
        for b in range(2):
            yield (f"dense b{b} hk1",) + both(st["grid"][b][1], lambda m: C.restate_stack64(st, pv, b, 1, m))
    elif mistake in ("batch_operands_of_batch_0", "interleave_b_h_swapped"):
        st = C.stack_slots(D, 456, False, gran)
        for lens in C.STACK_KV_LENS:
            for b, hk in ((1, 0), (1, 1)) if mistake == "batch_operands_of_batch_0" else ((0, 1), (1, 0)):
                own = C.cached_subcase(st["grid"][b][hk], None, lens[b])
                yield (f"kvlen {lens} b{b} hk{hk}",) + both(own, lambda m: C.restate_stack64(st, pv, b, hk, m, lens))
    elif mistake == "workspace_slot_of_head_0":
        st = C.stack_slots(D, 456, False, gran, anchored=True)
        km = C.stack_km(st)
        for b in range(2):
            for hk in range(2):
                own = st["grid"][b][hk]
                qkm = C.split_qkm(own, km[b:b + 1, hk:hk + 1])
                f = lambda m: C.restate_stack_split64(st, pv, 2, b, hk, None, qkm, m)
                g = lambda m: max(C.merged_ratios(own, pv, 2, *[x for i, x in enumerate(f(m)) if i != 1], qkm))
                yield f"splitkv S2 b{b} hk{hk}", g(None), g(mistake)
    elif mistake in ("cu_off_by_one_row", "scales_of_previous_sequence", "scale_row_by_max_seqlen_of_q"):
        for causal in (False, True):
            pk = C.pack_cases(D, gran, causal)
            for s, row in enumerate(pk["cases"]):
                for hk, own in enumerate(row):
                    if own["N"] and (s > 0 or mistake == "cu_off_by_one_row" or (hk > 0 and mistake == "scale_row_by_max_seqlen_of_q")):
                        yield (f"pack{'-causal' if causal else ''} seq{s} hk{hk}",) + both(own, lambda m: C.restate_pack64(pk, pv, s, hk, m))
    elif mistake == "causal_bottom_right":
        pk = C.pack_cases(D, gran, True)
        for s in (0, 2):
            for hk in range(2):
                yield (f"pack-causal seq{s} hk{hk}",) + both(pk["cases"][s][hk], lambda m: C.restate_pack64(pk, pv, s, hk, m))
        for label, c in C.causal_cut_cases(D, gran):
            yield (label,) + both(c, lambda m: C.restate_causal64(c, pv, m))
    else:
        tm = C.tile_major(C.stack_slots(D, 456, False, gran))
        for b in range(2):
            for hk in range(2):
                own = tm["st"]["grid"][b][hk]
                yield (f"tiles b{b} hk{hk}",) + both(own, lambda m: C.restate64(C.read_tiles(tm, b, hk, m), pv))


@pytest.mark.parametrize("mistake", C.LAYOUT_MISTAKES)
def test_layout_bound_has_teeth(mistake):
    """every deliberate addressing mistake of LAYOUT_MISTAKES leaves the bound (ratio > 1 on some element) on EVERY slice it
    should corrupt, at the shapes tests/test_constructed_layouts_gpu.py runs, while the same restatement without the mistake is
    the reference.  scale_row_by_max_seqlen_of_q cannot show where Gq(max M_s) = Gk(max N_s): per_warp scales at these lengths
    (8 groups each), stated here rather than hidden -- it shows under per_thread (64 against 32) and per_block (2 against 8)."""
    packed = mistake in C.LAYOUT_MISTAKES[4:7]
    for D, gran in LAYOUT_SHAPES:
        if mistake == "workspace_slot_of_head_0" and gran == "per_block":
            continue  # the fused-Q entry points have no per_block form
        if mistake == "scale_row_by_max_seqlen_of_q" and gran == "per_warp":
            pk = C.pack_cases(D, gran, False)
            assert pk["gq"] == pk["gk"] == 8
            continue
        for pv in ("fp16", "bf16") if packed else C.PVS:
            hit = 0
            for label, clean, r in _layout_mutants(mistake, D, gran, pv):
                print(f"layout teeth: {mistake:30s} {label:28s} {gran:10s} D={D:<3d} {pv:5s} ratio {r:12.4g}   (no mistake: {clean:.1e})")
                assert clean < 1e-3, (label, pv, clean)
                assert r > 1.0, (mistake, label, gran, D, pv, r)
                hit += 1
            assert hit > 0
