"""Strided views inside poisoned memory, shared by tests/test_strided_views.py (GPU) and tests/test_view_cases.py (CPU).

``make_input(kind, shape, dtype, seed)`` builds a logical ``[B,H,N,D]`` tensor and returns it as a view of a larger PARENT
allocation in which every byte that does not belong to the view is poison; ``make_output(kind, shape, dtype)`` returns a
view for a kernel to write whose parent holds a sentinel everywhere, inside the view as well.  Every kind is a valid C-ABI
tensor (include/sageattn_hip.h: unit last stride, 16-byte aligned base, strides multiples of 16 bytes), and each separates
one stride relation that a contiguous tensor ties to the sizes:

  packed_nhd        qkv[B,N,3,H,D].unbind(2), layout NHD              stride_n = 3HD instead of H*D
  packed_hnd        the same memory permuted to [B,H,N,D], layout HND  an HND call with stride_h = D, stride_n = 3HD
  seq_slice         parent[:, :, s0:s0+N], s0 not a multiple of 64     rows before 0 and past N are foreign
  seq_slice_nhd     the same cut of a [B,Ntot,H,D] buffer, layout NHD  a slice of a longer packed [T,H,D] buffer
  head_batch_slice  parent[1:, 1:-1]                                   stride_b != H * stride_h
  row_padded        wide[..., :D], rows 16 bytes longer                stride_n != D in HND
  kv_cache          cache[B,2,H,Nmax,D][:, which, :, :N]               K and V interleaved, tail rows foreign
  broadcast_b       x[:1].expand(B, ...)                               stride_b = 0 (inputs only)
  broadcast_h       x[:, :1].expand(-1, H, ...)                        stride_h = 0 (inputs only)

Poison: fp16 / bf16 inputs a seeded mix of quiet NaN and +Inf, int8 inputs 0x80, FP8 (e4m3) inputs 0x7f (NaN).  Output
sentinels: 0xff bytes for floating-point and FP8 outputs (NaN in fp16, bf16, fp32 and e4m3, so a value a kernel did not
write is never finite) and 0x80 for int8 outputs.  The one exception to "poison everywhere" is the FP8 V image
``[B,H,D,Npad]``: token columns in [N, Npad) are part of the view and must be ZERO (a contract of the FP8 V quantizer);
``fp8_image_input`` builds such an input, the tests assert the zeros where the image is an output."""
from typing import NamedTuple, Optional

import torch

INPUT_KINDS = ("packed_nhd", "packed_hnd", "seq_slice", "seq_slice_nhd", "head_batch_slice", "row_padded", "kv_cache",
               "broadcast_b", "broadcast_h")
OUTPUT_KINDS = INPUT_KINDS[:7]  # a view with a zero stride cannot be written
SEQ_START = 37                  # first row of a seq_slice inside its parent: not a multiple of 64

_FLOATS = (torch.float16, torch.bfloat16, torch.float32)


def out_sentinel(dtype) -> int:
    return 0x80 if dtype == torch.int8 else 0xFF


def poisoned(shape, dtype, seed):
    """A parent full of input poison."""
    if dtype in _FLOATS:
        g = torch.Generator().manual_seed(seed ^ 0x5EED)
        nan = torch.rand(shape, generator=g) < 0.5
        return torch.where(nan, torch.tensor(float("nan")), torch.tensor(float("inf"))).to(dtype)
    if dtype == torch.int8:
        return torch.full(shape, -128, dtype=torch.int8)
    if dtype == torch.float8_e4m3fn:
        return torch.full(shape, 0x7F, dtype=torch.uint8).view(torch.float8_e4m3fn)
    raise ValueError(dtype)


def sentinel(shape, dtype):
    n = 1
    for s in shape:
        n *= s
    return torch.full((n * dtype.itemsize,), out_sentinel(dtype), dtype=torch.uint8).view(dtype).view(shape)


def _ceil(n, m):
    return (n + m - 1) // m * m


def _carve(kind, parent_of, shape, dtype, seed):
    """-> (parent, [B,H,N,D] view of it, tensor layout the kind stands for)."""
    B, H, N, D = shape
    if kind in ("packed_nhd", "packed_hnd"):
        parent = parent_of((B, N, 3, H, D))
        return parent, parent[:, :, seed % 3].permute(0, 2, 1, 3), kind[-3:].upper()
    if kind == "seq_slice":
        parent = parent_of((B, H, SEQ_START + _ceil(N, 128) + 19, D))
        return parent, parent[:, :, SEQ_START:SEQ_START + N], "HND"
    if kind == "seq_slice_nhd":
        parent = parent_of((B, SEQ_START + _ceil(N, 128) + 19, H, D))
        return parent, parent[:, SEQ_START:SEQ_START + N].permute(0, 2, 1, 3), "NHD"
    if kind == "contiguous":  # the control: a fresh dense tensor, nothing around it
        parent = parent_of((B, H, N, D))
        return parent, parent, "HND"
    if kind == "head_batch_slice":
        parent = parent_of((B + 1, H + 2, N, D))
        return parent, parent[1:, 1:-1], "HND"
    if kind == "row_padded":
        parent = parent_of((B, H, N, D + 16 // dtype.itemsize))
        return parent, parent[..., :D], "HND"
    if kind == "kv_cache":
        parent = parent_of((B, 2, H, _ceil(N, 128) + 69, D))
        return parent, parent[:, seed % 2, :, :N], "HND"
    if kind == "broadcast_b":
        parent = parent_of((1, H, _ceil(N, 128) + 5, D))
        return parent, parent[:, :, :N].expand(B, H, N, D), "HND"
    if kind == "broadcast_h":
        parent = parent_of((B, 1, _ceil(N, 128) + 5, D))
        return parent, parent[:, :, :N].expand(B, H, N, D), "HND"
    raise ValueError(kind)


def byte_mask(view: torch.Tensor, parent: torch.Tensor) -> torch.Tensor:
    """bool [parent bytes]: the bytes of ``parent`` that ``view`` (any view of it) addresses, from the view's sizes and
    strides alone -- independent of how the view was carved."""
    assert parent.is_contiguous()
    isz = view.dtype.itemsize
    off = torch.full((1,) * view.dim(), view.storage_offset() - parent.storage_offset(), dtype=torch.int64)
    for d in range(view.dim()):
        idx = torch.arange(view.size(d), dtype=torch.int64) * view.stride(d)
        off = off + idx.view([-1 if i == d else 1 for i in range(view.dim())])
    off = off.reshape(-1) * isz
    assert int(off.min()) >= 0 and int(off.max()) + isz <= parent.numel() * isz
    mask = torch.zeros(parent.numel() * isz, dtype=torch.bool)
    for j in range(isz):
        mask[off + j] = True
    return mask


def raw_bytes(t: torch.Tensor) -> torch.Tensor:
    return t.reshape(-1).view(torch.uint8)


class View(NamedTuple):
    kind: str
    layout: str                 # the reference tensor_layout this kind stands for
    view: torch.Tensor          # [B,H,N,D] view of parent (strides = the sage_tensor strides)
    parent: torch.Tensor        # contiguous allocation
    mask: torch.Tensor          # bool per parent byte (CPU): belongs to the view
    before: torch.Tensor        # the parent's bytes at construction (CPU)
    logical: Optional[torch.Tensor]  # inputs: the values, [B,H,N,D] contiguous (CPU)

    def to(self, device) -> "View":
        parent = self.parent.to(device)
        v = self.view
        view = parent.as_strided(v.size(), v.stride(), v.storage_offset() - self.parent.storage_offset())
        return self._replace(view=view, parent=parent)

    def arg(self) -> torch.Tensor:
        """The tensor a Python operator takes together with ``tensor_layout=self.layout``."""
        return self.view if self.layout == "HND" else self.view.transpose(1, 2)

    def parent_unchanged(self) -> bool:
        return torch.equal(raw_bytes(self.parent).cpu(), self.before)

    def outside_untouched(self) -> bool:
        """Every byte of the parent outside the view still holds what it held at construction."""
        now = raw_bytes(self.parent).cpu()
        return torch.equal(now[~self.mask], self.before[~self.mask])

    def all_written(self) -> bool:
        """Floating-point and FP8 outputs: no element of the view still holds the (NaN) sentinel."""
        assert self.view.dtype != torch.int8
        v = self.view.contiguous().cpu()
        return not bool((raw_bytes(v).view(-1, v.dtype.itemsize) == 0xFF).all(dim=1).any())


def _finish(kind, layout, view, parent, logical):
    return View(kind, layout, view, parent, byte_mask(view, parent), raw_bytes(parent).clone(), logical)


def random_values(shape, dtype, seed, scale=1.0, channel_bias=0.0):
    """Seeded N(0, scale^2) values plus a per-channel offset; no channel is all zero."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * scale
    if channel_bias:
        x = x + channel_bias * torch.randn((1, shape[1], 1, shape[3]), generator=g)
    return x.to(dtype)


def make_input(kind, shape=None, dtype=torch.float16, seed=0, values=None, scale=1.0, channel_bias=0.0) -> View:
    """An input view of ``kind`` holding ``values`` ([B,H,N,D], any strides) or seeded random values of ``shape``.
    For the broadcast kinds the logical tensor repeats batch 0 / head 0 of the values."""
    if values is None:
        values = random_values(shape, dtype, seed, scale, channel_bias)
    values = values.cpu()
    shape, dtype = tuple(values.shape), values.dtype
    if kind == "broadcast_b":
        values = values[:1].expand(shape)
    elif kind == "broadcast_h":
        values = values[:, :1].expand(shape)
    parent, view, layout = _carve(kind, lambda s: poisoned(s, dtype, seed), shape, dtype, seed)
    if kind == "broadcast_b":
        parent[:, :, :shape[2]] = values[:1]
    elif kind == "broadcast_h":
        parent[:, :, :shape[2]] = values[:, :1]
    else:
        view.copy_(values)
    return _finish(kind, layout, view, parent, values.contiguous())


def make_output(kind, shape, dtype, seed=0) -> View:
    """An output view of ``kind``: the parent holds ``out_sentinel(dtype)`` bytes everywhere."""
    assert kind in OUTPUT_KINDS or kind == "contiguous", kind
    parent, view, layout = _carve(kind, lambda s: sentinel(s, dtype), tuple(shape), dtype, seed)
    return _finish(kind, layout, view, parent, None)


def fp8_image_input(kind, image: torch.Tensor, seed=0) -> View:
    """An FP8 V image ``[B,H,D,Npad]`` (float8_e4m3fn, zero in token columns >= N by contract) as an input view: the
    whole image, its zero columns included, is the view; foreign rows and columns >= Npad are 0x7f."""
    assert image.dtype == torch.float8_e4m3fn and image.shape[-1] % 64 == 0
    return make_input(kind, values=image, seed=seed)


def tensor_ok(view: torch.Tensor, align_bytes: int = 16) -> bool:
    """The C ABI's rule for a tensor argument (csrc/sage_common.h tensor_ok, at its strictest alignment)."""
    isz = view.dtype.itemsize
    return (view.stride(-1) == 1 and view.data_ptr() % 16 == 0
            and all((view.stride(d) * isz) % align_bytes == 0 for d in range(view.dim() - 1)))
