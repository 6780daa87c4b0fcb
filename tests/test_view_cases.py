"""CPU: the view catalogue of tests/view_cases.py itself -- a broken catalogue would make the GPU tests of
tests/test_strided_views.py vacuous.  Every kind must be a real strided view that the C ABI accepts, hold exactly its
logical values, be surrounded by poison, and give the oracle the same result as a contiguous copy."""
import pytest
import torch

import view_cases as V

SHAPE = (2, 3, 77, 64)


def _values(dtype, seed=11):
    if dtype in (torch.float16, torch.bfloat16):
        return None
    raw = torch.randint(-120, 120, SHAPE, dtype=torch.int8, generator=torch.Generator().manual_seed(seed))
    return raw if dtype == torch.int8 else (raw.view(torch.uint8) & 0x77).view(torch.float8_e4m3fn)  # finite e4m3 codes


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.int8, torch.float8_e4m3fn])
@pytest.mark.parametrize("kind", V.INPUT_KINDS)
def test_input_views(kind, dtype):
    c = V.make_input(kind, SHAPE, dtype, seed=11, values=_values(dtype))
    v = c.view
    assert tuple(v.shape) == SHAPE and v.dtype == dtype
    assert not v.is_contiguous() or 0 in v.stride()
    assert not v.transpose(1, 2).is_contiguous()
    assert V.tensor_ok(v), v.stride()
    assert torch.equal(V.raw_bytes(v.contiguous()), V.raw_bytes(c.logical))          # equals its logical tensor, bit for bit
    isz, numel = dtype.itemsize, v.numel()
    distinct = {"broadcast_b": numel // SHAPE[0], "broadcast_h": numel // SHAPE[1]}.get(kind, numel)
    assert int(c.mask.sum()) == distinct * isz and c.mask.numel() == c.parent.numel() * isz
    assert int((~c.mask).sum()) > 0
    # everything outside the view is poison, nothing inside is
    outside = c.before[~c.mask]
    if dtype in (torch.float16, torch.bfloat16):
        flat = c.parent.reshape(-1)
        elem_in = c.mask.view(-1, isz).all(dim=1)
        assert torch.equal(elem_in, c.mask.view(-1, isz).any(dim=1))
        assert torch.isfinite(flat[elem_in]).all() and not torch.isfinite(flat[~elem_in]).any()
        assert torch.isnan(flat[~elem_in]).any() and torch.isinf(flat[~elem_in]).any()  # both patterns
    else:
        assert (outside == (0x80 if dtype == torch.int8 else 0x7F)).all()
    assert c.parent_unchanged() and c.outside_untouched()
    # the layout form handed to the Python operators is the same tensor
    a = c.arg()
    assert a.data_ptr() == v.data_ptr() and (a.shape == v.shape if c.layout == "HND" else a.shape == v.transpose(1, 2).shape)
    # moving to a device keeps the geometry (the GPU tests rely on it)
    m = c.to("cpu")
    assert m.view.stride() == v.stride() and torch.equal(V.raw_bytes(m.view.contiguous()), V.raw_bytes(c.logical))


def test_kinds_separate_the_stride_relations_they_claim():
    B, H, N, D = SHAPE
    s = {k: V.make_input(k, SHAPE, torch.float16, seed=3).view.stride() for k in V.INPUT_KINDS}
    assert s["packed_nhd"] == (N * 3 * H * D, D, 3 * H * D, 1) and s["packed_hnd"] == s["packed_nhd"]
    assert V.make_input("packed_nhd", SHAPE, seed=3).layout == "NHD" and V.make_input("packed_hnd", SHAPE, seed=3).layout == "HND"
    c = V.make_input("seq_slice", SHAPE, torch.float16, seed=3)
    rows = c.parent.shape[2]
    assert V.SEQ_START % 64 != 0 and rows > V.SEQ_START + (N + 127) // 128 * 128
    assert s["head_batch_slice"][0] != H * s["head_batch_slice"][1]
    assert s["row_padded"][2] == D + 8
    c = V.make_input("kv_cache", SHAPE, torch.float16, seed=3)
    assert c.parent.shape[1] == 2 and c.parent.shape[3] >= (N + 127) // 128 * 128 + 64
    assert s["broadcast_b"][0] == 0 and s["broadcast_h"][1] == 0


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.int8, torch.float8_e4m3fn])
@pytest.mark.parametrize("kind", V.OUTPUT_KINDS)
def test_output_views(kind, dtype):
    c = V.make_output(kind, SHAPE, dtype)
    assert V.tensor_ok(c.view) and not c.view.is_contiguous()
    assert (c.before == V.out_sentinel(dtype)).all()
    assert int(c.mask.sum()) == c.view.numel() * dtype.itemsize
    if dtype != torch.int8:
        assert not c.all_written()
        if dtype in (torch.float16, torch.float32):
            assert torch.isnan(c.parent).all()
    # a write through the view changes the view's bytes only, and is seen
    if dtype in (torch.float16, torch.float32):
        c.view.copy_(torch.ones(SHAPE, dtype=dtype))
        assert c.all_written() and c.outside_untouched() and not c.parent_unchanged()
        c.parent.reshape(-1)[0 if not c.mask[0] else int((~c.mask).nonzero()[0]) // dtype.itemsize] = 1.0
        assert not c.outside_untouched()
        c.view[1, 2, 5, 7] = float("nan")
        c.view.view(torch.int16 if dtype == torch.float16 else torch.int32)[1, 2, 5, 7] = -1
        assert not c.all_written()


def test_fp8_image_input_keeps_the_zero_columns_inside_the_view():
    N, npad = 77, 128
    img = (torch.randint(0, 0x70, (2, 3, 64, npad), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)))
    img[..., N:] = 0
    c = V.fp8_image_input("row_padded", img.view(torch.float8_e4m3fn))
    got = c.view.view(torch.uint8)
    assert (got[..., N:] == 0).all() and torch.equal(got, img)
    assert (c.before[~c.mask] == 0x7F).all() and int(c.mask.sum()) == img.numel()


@pytest.mark.parametrize("kind", V.INPUT_KINDS)
def test_oracle_gives_the_same_result_on_a_view_as_on_its_copy(kind):
    from oracle import sage_oracle as O
    q = V.make_input(kind, (2, 4, 70, 64), torch.float16, seed=5)
    k = V.make_input(kind, (2, 2, 77, 64), torch.float16, seed=6, channel_bias=1.0)
    v = V.make_input(kind, (2, 2, 77, 64), torch.float16, seed=7)
    for pv in ("fp16", "fp8"):
        a = O.sageattn_oracle(q.arg(), k.arg(), v.arg(), tensor_layout=q.layout, pv=pv, return_lse=True)
        b = O.sageattn_oracle(q.arg().contiguous(), k.arg().contiguous(), v.arg().contiguous(), tensor_layout=q.layout,
                              pv=pv, return_lse=True)
        assert torch.isfinite(a[0]).all() and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    q8a, qsa, k8a, ksa = O.per_thread_int8(q.arg(), k.arg(), km=O.k_mean(k.arg(), k.layout), tensor_layout=k.layout)
    kc = k.arg().contiguous()
    q8b, qsb, k8b, ksb = O.per_thread_int8(q.arg().contiguous(), kc, km=O.k_mean(kc, k.layout), tensor_layout=k.layout)
    assert torch.equal(q8a, q8b) and torch.equal(qsa, qsb) and torch.equal(k8a, k8b) and torch.equal(ksa, ksb)
