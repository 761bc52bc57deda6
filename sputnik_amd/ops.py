"""Torch op surface over the block-sparse products, in the shape MegaBlocks
drives them: a topology object holding the BCSR
metadata once (plus the transposed metadata and row indices, built on the
device the first time a product needs them, so every later call is a
`MatmulEx`), and three differentiable ops

    sdd(a, b, topo) -> SparseMatrix   (a @ b at topo's nonzero blocks)
    dsd(a_sparse, b) -> Tensor        (op(a) @ b, a possibly a .t() view)
    dds(a, b_sparse) -> Tensor        (a @ op(b))

whose backward passes are again sdd / dsd / dds with transpose flags (the
MegaBlocks forward/backward set, BASELINE config 3). Each op takes optional
gradient sinks (`a_grad_out` / `b_grad_out`) for its dense operands: backward
then adds that operand's gradient into the sink with the accumulating product
(C += op(A) op(B), `dsd_acc` / `dds_acc` below) instead of returning it, the
Megatron `main_grad` convention.
`sdd_act(a, b, topo, activation)` is sdd with the activation
fused into the product, and `mlp(x, w1, w2, topo, activation)` the expert MLP
dsd(act(sdd(x, w1, topo)), w2) as one autograd function
(sputnik/block/activation.h). `sdd_gated(a, b, topo, gate, activation)` is
sdd multiplied by act(gate) in the product's epilogue, and `glu_mlp(x, w1, v1,
w2, topo, activation)` the gated expert MLP
dsd(act(sdd(x, w1, topo)) * sdd(x, v1, topo), w2) as one autograd function
(sputnik/block/gated.h). `moe_route`, `padded_gather` and `padded_scatter`
are the token permutation on either side of those MLPs (MegaBlocks'
padded_gather / padded_scatter; sputnik/block/moe.h), and `moe_mlp` the whole
layer behind a router: route, gather, expert topology, mlp / glu_mlp,
weighted scatter. `moe_router` is the router's fused softmax / top-k with its
gradient (sputnik/block/router.h), `moe_device_route` builds a route with the
library's counting sort instead of torch.sort, and `moe_layer` is the whole
layer from activations to output: router GEMM (torch), moe_router, moe_mlp.
`moe_router_aux` is moe_router with the fp32 statistics of the auxiliary
losses (column sums of the softmax, sum of logsumexp^2) taken in the same
pass, `load_balancing_loss` / `router_z_loss` the losses formed from them, and
`moe_layer_aux` the layer that returns those statistics beside its output.
`moe_score_router` is the router of models that score with a sigmoid, select
on score + bias and limit the choice to the best groups of experts
(RouterScoreTopK), `moe_score_layer` the layer routed by it and
`router_bias_update` the auxiliary-loss-free correction of that bias.
Expert biases (sputnik/block/bias.h) come as entry points of their own, each
named after the bias-free one and equal to it without a bias: `sdd_bias(a, b,
topo, bias)`, `sdd_act_bias` and `sdd_gated_bias` add a column bias in the
product's epilogue, `column_sum(sparse)` is its gradient, `mlp_bias(..., b1=)`
/ `glu_mlp_bias(..., b1=, bv1=)`, `padded_scatter_bias(..., bias=)` and
`moe_mlp_bias` / `moe_layer_bias` / `moe_layer_aux_bias` /
`moe_score_layer_bias(..., b1=, bv1=, b2=)` carry them through the expert
MLP and the scatter.
The fp8 forward path (sputnik/block/fp8.h; e4m3 elements with fp32 block
scales, forward only) is `quantize_rows`, `quantize_sparse` and
`quantize_weight` -> `Fp8Weight`, the products `sdd_fp8` / `dsd_fp8`, and
`moe_mlp_fp8`, moe_mlp with its expert products in fp8 while gather, scatter
and router stay 16-bit; the three take `accumulate="fp32"` (the default) or
`"fast"`, the scaled e4m3 MFMA per k-block (Fp8Accumulate in fp8.h).
The fp8 path with gradients is `mlp_fp8(x, w1t, w2, topo, activation)` over
16-bit tensors and `moe_mlp_fp8_train` around it; its pieces are
`quantize_tiles` (row and 128 x 1 column tiles in one pass),
`quantize_sparse_t` (a sparse operand's transpose with per-column scales),
`Fp8Weight.t()` and `dsd_fp8_wgrad`, the DSD whose dense operand is scaled
per column.
Every product runs on
libsputnik.so through the C-ABI on the current torch stream; there is no
dense or CPU fallback (a missing library raises).

The BCSR wire format is the reference's `BlockMatrix` (arguments.h:48-153):
`data` holds #blocks row-major 128x128 blocks ([nb, 128, 128] here),
`offsets` int32 [rows/128 + 1] in blocks, `indices` int16 [nb] block
columns; `offsets_t` / `indices_t` / `block_offsets` are what
`Transpose` (transpose.cu:69-125) produces and `row_indices` what
`RowIndices` (row_indices.cu:7-36) produces.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import (BlockActivation, BlockActivationGrad, BlockGate, BlockGateGrad,
               BlockMatrix, Matrix, Matmul, MatmulAccumulateEx,
               MatmulActivation, MatmulActivationGrad, MatmulEx, MatmulGated,
               MatmulGatedGrad, MoeBins, MoeRowMap, MoeSort, PaddedGather,
               PaddedScatter, PaddedScatterWeightGrad, RouterTopK,
               BlockColumnSum, MatmulBias, MatmulBiasActivation,
               MatmulBiasGated, PaddedScatterBias, PaddedScatterBiasGrad,
               PaddedScatterBiasWeightGrad,
               QuantizeRows, QuantizeWeight, SddFp8, DsdFp8, FP8_ACCUMULATE,
               QuantizeTiles, QuantizeBlocks, TransposeWeightFp8, DsdFp8Wgrad,
               RouterScoreTopK, RouterScoreTopKGrad, RouterTopKAux,
               RouterTopKAuxGrad, RouterTopKGrad, RowIndices, Transpose,
               MOE_SORT_CHUNK, ROUTER_AUX_TOKENS, ROUTER_MAX_EXPERTS,
               ROUTER_MAX_GROUPS, ROUTER_MAX_TOP_K, _act_code,
               AllocateRowIndicesBuffer, AllocateTransposeBuffers,
               dsd_workspace_bytes, sdd_workspace_bytes)

BLOCK = 128


class _Meta:
    """Device metadata shared by every view of one topology."""

    def __init__(self, rows, cols, offsets, indices):
        self.rows, self.cols = rows, cols
        self.offsets = offsets
        self.indices = indices
        self.offsets_t = None
        self.indices_t = None
        self.block_offsets = None
        self.row_indices = None
        self.nb = int(indices.numel())

    def descriptor(self, data) -> BlockMatrix:
        return BlockMatrix(self.rows, self.cols, BLOCK, self.nb * BLOCK * BLOCK,
                           data, self.offsets, self.indices, self.offsets_t,
                           self.indices_t, self.block_offsets, self.row_indices)

    def ensure_transposed(self, data):
        if self.offsets_t is None:
            d = self.descriptor(data)
            AllocateTransposeBuffers(d)
            Transpose(d)
            self.offsets_t, self.indices_t = d.offsets_t, d.indices_t
            self.block_offsets = d.block_offsets

    def ensure_row_indices(self, data):
        if self.row_indices is None:
            d = self.descriptor(data)
            AllocateRowIndicesBuffer(d)
            RowIndices(d, d.row_indices)
            self.row_indices = d.row_indices


class SparseMatrix:
    """A block-sparse matrix (128x128 blocks). `shape` is the logical shape;
    a `.t()` view shares data and metadata and flips the transpose flag the
    products receive, as MegaBlocks/stk's transposed views do."""

    def __init__(self, size: Tuple[int, int], data: torch.Tensor,
                 offsets: torch.Tensor, indices: torch.Tensor,
                 _meta: Optional[_Meta] = None, _transposed: bool = False):
        rows, cols = int(size[0]), int(size[1])
        if rows % BLOCK or cols % BLOCK:
            raise ValueError(f"sparse shape {size} is not a multiple of 128")
        if data.dim() != 3 or tuple(data.shape[1:]) != (BLOCK, BLOCK):
            raise ValueError("data must be [#blocks, 128, 128]")
        if data.shape[0] != indices.numel():
            raise ValueError("data and indices disagree on #blocks")
        if offsets.dtype != torch.int32 or indices.dtype != torch.int16:
            raise TypeError("offsets int32, indices int16 (arguments.h:48-153)")
        if offsets.numel() != rows // BLOCK + 1:
            raise ValueError("offsets must have rows/128 + 1 entries")
        self.data = data
        self._meta = _meta or _Meta(rows, cols, offsets.contiguous(),
                                    indices.contiguous())
        self._transposed = _transposed

    # -- views ------------------------------------------------------------
    @property
    def shape(self):
        m = self._meta
        return (m.cols, m.rows) if self._transposed else (m.rows, m.cols)

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    @property
    def dtype(self):
        return self.data.dtype

    @property
    def device(self):
        return self.data.device

    @property
    def offsets(self):
        return self._meta.offsets

    @property
    def indices(self):
        return self._meta.indices

    @property
    def nnz_blocks(self) -> int:
        return self._meta.nb

    def is_transposed(self) -> bool:
        return self._transposed

    def t(self) -> "SparseMatrix":
        return SparseMatrix((self._meta.rows, self._meta.cols), self.data,
                            self._meta.offsets, self._meta.indices,
                            _meta=self._meta, _transposed=not self._transposed)

    def with_data(self, data: torch.Tensor) -> "SparseMatrix":
        """Same topology (and view), new block values."""
        return SparseMatrix((self._meta.rows, self._meta.cols), data,
                            self._meta.offsets, self._meta.indices,
                            _meta=self._meta, _transposed=self._transposed)

    def to_dense(self) -> torch.Tensor:
        """Dense copy (block scatter with torch indexing; test/debug aid)."""
        m = self._meta
        rb, cb = m.rows // BLOCK, m.cols // BLOCK
        counts = (m.offsets[1:] - m.offsets[:-1]).long()
        rows = torch.repeat_interleave(torch.arange(rb, device=self.device),
                                       counts)
        cols = m.indices.long()
        out = torch.zeros(rb, cb, BLOCK, BLOCK, dtype=self.dtype,
                          device=self.device)
        out[rows, cols] = self.data
        dense = out.permute(0, 2, 1, 3).reshape(m.rows, m.cols)
        return dense.t() if self._transposed else dense

    def _descriptor(self) -> BlockMatrix:
        return self._meta.descriptor(self.data)


# ---- dense operand plumbing -------------------------------------------------

def _dense_operand(x: torch.Tensor) -> Tuple[Matrix, bool]:
    """(stored matrix, transpose flag) for a 2-D tensor: a transposed view of
    a contiguous tensor is passed as the stored matrix with the flag set,
    anything else is made contiguous."""
    if x.dim() != 2:
        raise ValueError("dense operands are 2-D")
    if x.is_contiguous():
        return Matrix(x.shape[0], x.shape[1], x), False
    if x.t().is_contiguous():
        s = x.t()
        return Matrix(s.shape[0], s.shape[1], s), True
    x = x.contiguous()
    return Matrix(x.shape[0], x.shape[1], x), False


def _check_dtypes(*ts):
    dt = ts[0].dtype
    if dt not in (torch.float16, torch.bfloat16):
        raise TypeError(f"unsupported dtype {dt} (fp16 or bf16)")
    for t in ts[1:]:
        if t.dtype != dt:
            raise TypeError("operands must share one dtype")


# ---- raw products (no autograd) ---------------------------------------------

def _bt_workspace(nbytes: int, device) -> Optional[torch.Tensor]:
    """Memory for the transposed copy of B when a product asks for it: a
    per-call temporary from torch's caching allocator, so the library never
    allocates a buffer of its own for these ops. The allocator's stream
    ordering makes its reuse safe in eager mode; under torch.cuda.graph it
    comes from the graph's private pool and lives as long as the graph."""
    if nbytes == 0:
        return None
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _dsd(a: SparseMatrix, b: torch.Tensor) -> torch.Tensor:
    _check_dtypes(a.data, b)
    if a.shape[1] != b.shape[0]:
        raise ValueError(f"dsd shapes {a.shape} x {tuple(b.shape)}")
    bm, tb = _dense_operand(b)
    out = torch.empty(a.shape[0], b.shape[1], dtype=b.dtype, device=b.device)
    if a.is_transposed():
        a._meta.ensure_transposed(a.data)
    ad, om = a._descriptor(), Matrix(out.shape[0], out.shape[1], out)
    ws = _bt_workspace(dsd_workspace_bytes(ad, a.is_transposed(), bm, tb, om),
                       b.device)
    MatmulEx(ad, a.is_transposed(), bm, tb, om, workspace=ws)
    return out


def _dds(a: torch.Tensor, b: SparseMatrix) -> torch.Tensor:
    _check_dtypes(a, b.data)
    if a.shape[1] != b.shape[0]:
        raise ValueError(f"dds shapes {tuple(a.shape)} x {b.shape}")
    am, ta = _dense_operand(a)
    out = torch.empty(a.shape[0], b.shape[1], dtype=a.dtype, device=a.device)
    if not b.is_transposed():  # row n of op(B)^T is column n of B
        b._meta.ensure_transposed(b.data)
    MatmulEx(am, ta, b._descriptor(), b.is_transposed(),
             Matrix(out.shape[0], out.shape[1], out))
    return out


def _sdd_setup(a: torch.Tensor, b: torch.Tensor, topo: SparseMatrix):
    """What every SDD form passes to the library: (am, ta, bm, tb, cd, ws,
    data), `data` the new block values cd describes. A transposed topo view
    means the product is stored transposed: (a @ b)^T = b^T @ a^T is computed
    instead."""
    _check_dtypes(a, b)
    if a.shape[1] != b.shape[0] or (a.shape[0], b.shape[1]) != topo.shape:
        raise ValueError(f"sdd shapes {tuple(a.shape)} x {tuple(b.shape)} "
                         f"-> {topo.shape}")
    if topo.is_transposed():
        a, b = b.t(), a.t()
    am, ta = _dense_operand(a)
    bm, tb = _dense_operand(b)
    data = torch.empty(topo.nnz_blocks, BLOCK, BLOCK, dtype=a.dtype,
                       device=a.device)
    topo._meta.ensure_row_indices(data)
    cd = topo._meta.descriptor(data)
    ws = _bt_workspace(sdd_workspace_bytes(am, ta, bm, tb, cd), a.device)
    return am, ta, bm, tb, cd, ws, data


def _sdd(a: torch.Tensor, b: torch.Tensor, topo: SparseMatrix,
         bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Block values of (a @ b) at topo's nonzero blocks, in topo's storage
    order; with `bias`, of round(a @ b) + bias[col] (MatmulBias)."""
    am, ta, bm, tb, cd, ws, data = _sdd_setup(a, b, topo)
    if bias is None:
        Matmul(am, ta, bm, tb, cd, workspace=ws)
    else:
        MatmulBias(am, ta, bm, tb, cd, bias, workspace=ws)
    return data


def _check_bias(bias, ref: torch.Tensor, shape: tuple, what: str):
    """An expert bias: a tensor of `shape`, of ref's dtype and device."""
    if not isinstance(bias, torch.Tensor):
        raise TypeError(f"{what} must be a tensor")
    if bias.dtype != ref.dtype:
        raise TypeError(f"{what} is {bias.dtype}, expected {ref.dtype}")
    if bias.device != ref.device:
        raise ValueError(f"{what} is on {bias.device}, expected {ref.device}")
    if tuple(bias.shape) != tuple(shape):
        raise ValueError(f"{what} has shape {tuple(bias.shape)}, expected "
                         f"{tuple(shape)}")


def _column_bias(bias, ref: torch.Tensor, topo: SparseMatrix, what: str):
    """A column bias of an SDD into topo (None passes): [topo's columns] of
    ref's dtype and device, made contiguous. The bias is indexed by the
    stored matrix's columns, so a transposed topo view takes none."""
    if bias is None:
        return None
    if topo.is_transposed():
        raise ValueError(f"{what}: a bias needs a topo that is not a .t() "
                         "view")
    _check_bias(bias, ref, (topo.shape[1],), what)
    return bias.contiguous()


def _column_sum(data: torch.Tensor, topo: SparseMatrix) -> torch.Tensor:
    """fp32 [columns]: the column sums of topo's blocks with values `data`
    (BlockColumnSum)."""
    topo._meta.ensure_transposed(data)
    out = torch.empty(topo._meta.cols, dtype=torch.float32,
                      device=data.device)
    BlockColumnSum(topo._meta.descriptor(data), out)
    return out


def _sdd_act(a: torch.Tensor, b: torch.Tensor, topo: SparseMatrix, act: int,
             z: Optional[torch.Tensor] = None, grad: bool = False,
             keep_z: bool = False, bias: Optional[torch.Tensor] = None):
    """_sdd with the activation epilogue (MatmulActivation[Grad]). Forward
    (grad False): returns (H, Z), Z None unless keep_z; with `bias`, Z is the
    biased product (MatmulBiasActivation). Gradient: returns round(a @ b) *
    act'(z) at topo's blocks."""
    am, ta, bm, tb, cd, ws, data = _sdd_setup(a, b, topo)
    if grad:
        MatmulActivationGrad(am, ta, bm, tb, cd, act, z, workspace=ws)
        return data
    z = torch.empty_like(data) if keep_z else None
    if bias is None:
        MatmulActivation(am, ta, bm, tb, cd, act, z, workspace=ws)
    else:
        MatmulBiasActivation(am, ta, bm, tb, cd, bias, act, z, workspace=ws)
    return data, z


def _sdd_gated(a: torch.Tensor, b: torch.Tensor, topo: SparseMatrix, act: int,
               gate: torch.Tensor, up: Optional[torch.Tensor] = None,
               grad: bool = False, keep_up: bool = False,
               bias: Optional[torch.Tensor] = None):
    """_sdd with the gated epilogue (MatmulGated[Grad]); `gate` is G's block
    data. Forward (grad False): returns (H, U), U None unless keep_up; with
    `bias`, U is the biased product (MatmulBiasGated). Gradient: returns
    (dG, dU) of D = a @ b, dU written over `up`."""
    am, ta, bm, tb, cd, ws, data = _sdd_setup(a, b, topo)
    if grad:
        MatmulGatedGrad(am, ta, bm, tb, cd, act, gate, up, up, workspace=ws)
        return data, up
    up = torch.empty_like(data) if keep_up else None
    if bias is None:
        MatmulGated(am, ta, bm, tb, cd, act, gate, up, workspace=ws)
    else:
        MatmulBiasGated(am, ta, bm, tb, cd, bias, act, gate, up, workspace=ws)
    return data, up


# ---- accumulating products (no autograd) ------------------------------------

def _check_sink(out: torch.Tensor, rows: int, cols: int, dt, what: str):
    if not isinstance(out, torch.Tensor) or out.dim() != 2:
        raise TypeError(f"{what}: the sink must be a 2-D tensor")
    if tuple(out.shape) != (rows, cols):
        raise ValueError(f"{what}: sink shape {tuple(out.shape)}, expected "
                         f"{(rows, cols)}")
    if not out.is_contiguous():
        raise ValueError(f"{what}: the sink must be contiguous")
    if out.dtype not in (dt, torch.float32):
        raise TypeError(f"{what}: sink dtype {out.dtype}, expected {dt} or "
                        "torch.float32")


def dsd_acc(a: SparseMatrix, b: torch.Tensor, out: torch.Tensor
            ) -> torch.Tensor:
    """out += op(a_sparse) @ b in place, rounded once after the add; `out`
    is contiguous, of b's dtype or fp32, and must not overlap a or b. Rows of
    `out` that meet no block of op(a) are not touched. Returns `out`."""
    _check_dtypes(a.data, b)
    if a.shape[1] != b.shape[0]:
        raise ValueError(f"dsd shapes {a.shape} x {tuple(b.shape)}")
    _check_sink(out, a.shape[0], b.shape[1], b.dtype, "dsd_acc")
    bm, tb = _dense_operand(b)
    if a.is_transposed():
        a._meta.ensure_transposed(a.data)
    MatmulAccumulateEx(a._descriptor(), a.is_transposed(), bm, tb,
                       Matrix(out.shape[0], out.shape[1], out))
    return out


def dds_acc(a: torch.Tensor, b: SparseMatrix, out: torch.Tensor
            ) -> torch.Tensor:
    """out += a @ op(b_sparse) in place (as dsd_acc); columns of `out` that
    meet no block of op(b) are not touched. Returns `out`."""
    _check_dtypes(a, b.data)
    if a.shape[1] != b.shape[0]:
        raise ValueError(f"dds shapes {tuple(a.shape)} x {b.shape}")
    _check_sink(out, a.shape[0], b.shape[1], a.dtype, "dds_acc")
    am, ta = _dense_operand(a)
    if not b.is_transposed():  # row n of op(B)^T is column n of B
        b._meta.ensure_transposed(b.data)
    MatmulAccumulateEx(am, ta, b._descriptor(), b.is_transposed(),
                       Matrix(out.shape[0], out.shape[1], out))
    return out


class _Sink:
    """A gradient sink of one dense operand. The sink belongs to the tensor
    the caller holds: when the operand reached the op as a transposed view of
    a contiguous tensor, the sink has that tensor's shape and receives the
    transposed gradient."""

    def __init__(self, out: torch.Tensor, operand: torch.Tensor, what: str):
        self.out = out
        self.transposed = (operand.dim() == 2 and not operand.is_contiguous()
                           and operand.t().is_contiguous())
        rows, cols = operand.shape
        if self.transposed:
            rows, cols = cols, rows
        _check_sink(out, rows, cols, operand.dtype, what)

    # (X Y)^T = Y^T X^T: the transposed product swaps DSD and DDS and flips
    # both operands' flags, so no transposing copy is made.
    def add_dsd(self, a: SparseMatrix, b: torch.Tensor):
        if self.transposed:
            dds_acc(b.t(), a.t(), self.out)
        else:
            dsd_acc(a, b, self.out)

    def add_dds(self, a: torch.Tensor, b: SparseMatrix):
        if self.transposed:
            dsd_acc(b.t(), a.t(), self.out)
        else:
            dds_acc(a, b, self.out)


def _sink(out, operand, what):
    return None if out is None else _Sink(out, operand, what)


# ---- autograd ---------------------------------------------------------------

class _DSD(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a_data, b, a, b_sink):
        ctx.a = a
        ctx.b_sink = b_sink
        ctx.save_for_backward(a_data, b)
        return _dsd(a.with_data(a_data), b)

    @staticmethod
    def backward(ctx, dc):
        a_data, b = ctx.saved_tensors
        a = ctx.a.with_data(a_data)
        da = db = None
        if ctx.b_sink is not None:
            ctx.b_sink.add_dsd(a.t(), dc)              # sink += op(A)^T dC
        elif ctx.needs_input_grad[1]:
            db = _dsd(a.t(), dc)                       # op(A)^T dC
        if ctx.needs_input_grad[0]:
            # C = S B: dS = dC B^T;  C = S^T B: dS = B dC^T (at S's blocks)
            stored = a.t() if a.is_transposed() else a
            da = (_sdd(b, dc.t(), stored) if a.is_transposed()
                  else _sdd(dc, b.t(), stored))
        return da, db, None, None


class _DDS(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b_data, b, a_sink):
        ctx.b = b
        ctx.a_sink = a_sink
        ctx.save_for_backward(a, b_data)
        return _dds(a, b.with_data(b_data))

    @staticmethod
    def backward(ctx, dc):
        a, b_data = ctx.saved_tensors
        b = ctx.b.with_data(b_data)
        da = db = None
        if ctx.a_sink is not None:
            ctx.a_sink.add_dds(dc, b.t())              # sink += dC op(B)^T
        elif ctx.needs_input_grad[0]:
            da = _dds(dc, b.t())                       # dC op(B)^T
        if ctx.needs_input_grad[1]:
            # C = A S: dS = A^T dC;  C = A S^T: dS = dC^T A (at S's blocks)
            stored = b.t() if b.is_transposed() else b
            db = (_sdd(dc.t(), a, stored) if b.is_transposed()
                  else _sdd(a.t(), dc, stored))
        return da, db, None, None


class _SDD(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, topo, a_sink, b_sink, bias=None):
        ctx.topo = topo
        ctx.a_sink, ctx.b_sink = a_sink, b_sink
        ctx.save_for_backward(a, b)
        ctx.bias_dtype = None if bias is None else bias.dtype
        return _sdd(a, b, topo, bias)

    @staticmethod
    def backward(ctx, dc_data):
        a, b = ctx.saved_tensors
        dc = ctx.topo.with_data(dc_data.contiguous())
        da = db = None
        if ctx.a_sink is not None:
            ctx.a_sink.add_dsd(dc, b.t())              # sink += dC B^T
        elif ctx.needs_input_grad[0]:
            da = _dsd(dc, b.t())                       # dC B^T
        if ctx.b_sink is not None:
            ctx.b_sink.add_dds(a.t(), dc)              # sink += A^T dC
        elif ctx.needs_input_grad[1]:
            db = _dds(a.t(), dc)                       # A^T dC
        dbias = None
        if ctx.bias_dtype is not None and ctx.needs_input_grad[5]:
            dbias = _column_sum(dc.data, ctx.topo).to(ctx.bias_dtype)
        return da, db, None, None, None, dbias


class _SDDAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, topo, act, a_sink, b_sink, bias=None):
        ctx.topo, ctx.act = topo, act
        ctx.a_sink, ctx.b_sink = a_sink, b_sink
        ctx.bias_dtype = None if bias is None else bias.dtype
        # (Z is stored only when a backward pass can follow)
        keep = (any(ctx.needs_input_grad[:2]) or a_sink is not None
                or b_sink is not None
                or (bias is not None and ctx.needs_input_grad[6]))
        h, z = _sdd_act(a, b, topo, act, keep_z=keep, bias=bias)
        if keep:
            ctx.save_for_backward(a, b, z)
        return h

    @staticmethod
    def backward(ctx, dh_data):
        a, b, z = ctx.saved_tensors
        # dZ = dH * act'(Z), then as _SDD.backward
        dz = BlockActivationGrad(dh_data.contiguous(), z, ctx.act)
        dc = ctx.topo.with_data(dz)
        da = db = None
        if ctx.a_sink is not None:
            ctx.a_sink.add_dsd(dc, b.t())              # sink += dZ B^T
        elif ctx.needs_input_grad[0]:
            da = _dsd(dc, b.t())                       # dZ B^T
        if ctx.b_sink is not None:
            ctx.b_sink.add_dds(a.t(), dc)              # sink += A^T dZ
        elif ctx.needs_input_grad[1]:
            db = _dds(a.t(), dc)                       # A^T dZ
        dbias = None
        if ctx.bias_dtype is not None and ctx.needs_input_grad[6]:
            dbias = _column_sum(dz, ctx.topo).to(ctx.bias_dtype)
        return da, db, None, None, None, None, dbias


class _MLP(torch.autograd.Function):
    """y = dsd(act(sdd(x, w1, topo)), w2). Keeps Z, not H: H = act(Z) is
    recomputed in backward, bit for bit what forward multiplied by w2."""

    @staticmethod
    def forward(ctx, x, w1, w2, topo, act, w1_sink, w2_sink, b1=None):
        ctx.topo, ctx.act = topo, act
        ctx.w1_sink, ctx.w2_sink = w1_sink, w2_sink
        # (the bias is not kept: backward needs its dtype alone)
        ctx.b1 = b1 is not None and ctx.needs_input_grad[7] and b1.dtype
        keep = (any(ctx.needs_input_grad[:3]) or w1_sink is not None
                or w2_sink is not None or bool(ctx.b1))
        h, z = _sdd_act(x, w1, topo, act, keep_z=keep, bias=b1)
        if keep:
            ctx.save_for_backward(x, w1, w2, z)
        return _dsd(topo.with_data(h), w2)

    @staticmethod
    def backward(ctx, dy):
        x, w1, w2, z = ctx.saved_tensors
        topo = ctx.topo
        dx = dw1 = dw2 = db1 = None
        if ctx.w2_sink is not None or ctx.needs_input_grad[2]:
            h = topo.with_data(BlockActivation(z, ctx.act))
            if ctx.w2_sink is not None:
                ctx.w2_sink.add_dsd(h.t(), dy)         # sink += H^T dY
            else:
                dw2 = _dsd(h.t(), dy)                  # H^T dY
            del h
        if (ctx.w1_sink is not None or ctx.needs_input_grad[0]
                or ctx.needs_input_grad[1] or ctx.b1):
            # dZ = (dY W2^T) * act'(Z), one product
            dz = topo.with_data(_sdd_act(dy, w2.t(), topo, ctx.act, z=z,
                                         grad=True))
            if ctx.needs_input_grad[0]:
                dx = _dsd(dz, w1.t())                  # dZ W1^T
            if ctx.w1_sink is not None:
                ctx.w1_sink.add_dds(x.t(), dz)         # sink += X^T dZ
            elif ctx.needs_input_grad[1]:
                dw1 = _dds(x.t(), dz)                  # X^T dZ
            if ctx.b1:
                db1 = _column_sum(dz.data, topo).to(ctx.b1)
        return dx, dw1, dw2, None, None, None, None, db1


class _SDDGated(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, gate_data, topo, act, a_sink, b_sink, bias=None):
        ctx.topo, ctx.act = topo, act
        ctx.a_sink, ctx.b_sink = a_sink, b_sink
        ctx.bias_dtype = None if bias is None else bias.dtype
        # (U is stored only when a backward pass can follow)
        keep = (any(ctx.needs_input_grad[:3]) or a_sink is not None
                or b_sink is not None
                or (bias is not None and ctx.needs_input_grad[7]))
        g = gate_data.contiguous()
        h, u = _sdd_gated(a, b, topo, act, g, keep_up=keep, bias=bias)
        if keep:
            ctx.save_for_backward(a, b, g, u)
        return h

    @staticmethod
    def backward(ctx, dh_data):
        a, b, g, u = ctx.saved_tensors
        # dG = dH U act'(G), dU = dH act(G), then as _SDD.backward on dU
        dg, du = BlockGateGrad(dh_data.contiguous(), g, u, ctx.act)
        dc = ctx.topo.with_data(du)
        da = db = None
        if ctx.a_sink is not None:
            ctx.a_sink.add_dsd(dc, b.t())              # sink += dU B^T
        elif ctx.needs_input_grad[0]:
            da = _dsd(dc, b.t())                       # dU B^T
        if ctx.b_sink is not None:
            ctx.b_sink.add_dds(a.t(), dc)              # sink += A^T dU
        elif ctx.needs_input_grad[1]:
            db = _dds(a.t(), dc)                       # A^T dU
        if not ctx.needs_input_grad[2]:
            dg = None
        dbias = None
        if ctx.bias_dtype is not None and ctx.needs_input_grad[7]:
            dbias = _column_sum(du, ctx.topo).to(ctx.bias_dtype)
        return da, db, dg, None, None, None, None, dbias


class _GLUMLP(torch.autograd.Function):
    """y = dsd(act(sdd(x, w1)) * sdd(x, v1), w2). Keeps Z1 = x w1 and
    Z2 = x v1, not H: H is recomputed from them in backward, bit for bit what
    forward multiplied by w2, and dZ2 is written over Z2."""

    @staticmethod
    def forward(ctx, x, w1, v1, w2, topo, act, w1_sink, v1_sink, w2_sink,
                b1=None, bv1=None):
        ctx.topo, ctx.act = topo, act
        ctx.w1_sink, ctx.v1_sink, ctx.w2_sink = w1_sink, v1_sink, w2_sink
        # (the biases are not kept: backward needs their dtypes alone)
        ctx.b1 = b1 is not None and ctx.needs_input_grad[9] and b1.dtype
        ctx.bv1 = bv1 is not None and ctx.needs_input_grad[10] and bv1.dtype
        keep = (any(ctx.needs_input_grad[:4]) or w1_sink is not None
                or v1_sink is not None or w2_sink is not None
                or bool(ctx.b1) or bool(ctx.bv1))
        z1 = _sdd(x, w1, topo, b1)
        h, z2 = _sdd_gated(x, v1, topo, act, z1, keep_up=keep, bias=bv1)
        if keep:
            ctx.save_for_backward(x, w1, v1, w2, z1, z2)
        return _dsd(topo.with_data(h), w2)

    @staticmethod
    def backward(ctx, dy):
        x, w1, v1, w2, z1, z2 = ctx.saved_tensors
        topo = ctx.topo
        dx = dw1 = dv1 = dw2 = db1 = dbv1 = None
        if ctx.w2_sink is not None or ctx.needs_input_grad[3]:
            h = topo.with_data(BlockGate(z2, z1, ctx.act))
            if ctx.w2_sink is not None:
                ctx.w2_sink.add_dsd(h.t(), dy)         # sink += H^T dY
            else:
                dw2 = _dsd(h.t(), dy)                  # H^T dY
            del h
        if (ctx.w1_sink is not None or ctx.v1_sink is not None
                or any(ctx.needs_input_grad[:3]) or ctx.b1 or ctx.bv1):
            # D = dY W2^T: dZ1 = D Z2 act'(Z1), dZ2 = D act(Z1) over Z2, one
            # product. Z2 is gone after it, so this node runs backward once.
            if getattr(ctx, "z2_consumed", False):
                raise RuntimeError("glu_mlp: backward ran before and wrote "
                                   "dZ2 over the saved Z2; call glu_mlp again")
            ctx.z2_consumed = True
            dz1, dz2 = _sdd_gated(dy, w2.t(), topo, ctx.act, z1, up=z2,
                                  grad=True)
            dz1, dz2 = topo.with_data(dz1), topo.with_data(dz2)
            if ctx.needs_input_grad[0]:
                dx = _dsd(dz1, w1.t())                 # dZ1 W1^T
                dsd_acc(dz2, v1.t(), dx)               # += dZ2 V1^T
            if ctx.w1_sink is not None:
                ctx.w1_sink.add_dds(x.t(), dz1)        # sink += X^T dZ1
            elif ctx.needs_input_grad[1]:
                dw1 = _dds(x.t(), dz1)                 # X^T dZ1
            if ctx.v1_sink is not None:
                ctx.v1_sink.add_dds(x.t(), dz2)        # sink += X^T dZ2
            elif ctx.needs_input_grad[2]:
                dv1 = _dds(x.t(), dz2)                 # X^T dZ2
            if ctx.b1:
                db1 = _column_sum(dz1.data, topo).to(ctx.b1)
            if ctx.bv1:
                dbv1 = _column_sum(dz2.data, topo).to(ctx.bv1)
        return (dx, dw1, dv1, dw2, None, None, None, None, None, db1, dbv1)


# Gradient sinks (`*_grad_out`): a contiguous tensor of the dense operand's
# shape (of the tensor the caller holds when the operand is its .t() view),
# in the operand's dtype or fp32. Backward adds the operand's gradient into
# it with the accumulating product, allocates no gradient-sized temporary
# and returns None for that operand, so its .grad stays unset. The sink must
# not overlap any operand or the incoming gradient. Without sinks nothing
# changes.

def dsd(a: SparseMatrix, b: torch.Tensor,
        b_grad_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Dense = op(sparse) @ dense (reference dsd.h:10-22)."""
    return _DSD.apply(a.data, b, a, _sink(b_grad_out, b, "dsd b_grad_out"))


def dds(a: torch.Tensor, b: SparseMatrix,
        a_grad_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Dense = dense @ op(sparse) (reference dds.h:10-22)."""
    return _DDS.apply(a, b.data, b, _sink(a_grad_out, a, "dds a_grad_out"))


def sdd(a: torch.Tensor, b: torch.Tensor, topo: SparseMatrix,
        a_grad_out: Optional[torch.Tensor] = None,
        b_grad_out: Optional[torch.Tensor] = None) -> SparseMatrix:
    """Sparse (topo's blocks) = dense @ dense (reference sdd.h:10-15)."""
    return topo.with_data(_SDD.apply(
        a, b, topo, _sink(a_grad_out, a, "sdd a_grad_out"),
        _sink(b_grad_out, b, "sdd b_grad_out"), None))


def sdd_bias(a: torch.Tensor, b: torch.Tensor, topo: SparseMatrix,
             bias: torch.Tensor,
             a_grad_out: Optional[torch.Tensor] = None,
             b_grad_out: Optional[torch.Tensor] = None) -> SparseMatrix:
    """Sparse (topo's blocks) = dense @ dense + bias[column], the bias added
    in the product's epilogue (MatmulBias): `bias` is [topo's columns] of the
    operands' dtype, and the result is round(a @ b) + bias rounded once more.
    Differentiable in a, b and bias (column_sum of the incoming gradient)."""
    if bias is None:
        raise TypeError("sdd_bias needs a bias; sdd is the bias-free product")
    return topo.with_data(_SDD.apply(
        a, b, topo, _sink(a_grad_out, a, "sdd_bias a_grad_out"),
        _sink(b_grad_out, b, "sdd_bias b_grad_out"),
        _column_bias(bias, a, topo, "sdd_bias: bias")))


def column_sum(sparse: SparseMatrix) -> torch.Tensor:
    """fp32 [columns]: the sum of every column of `sparse` over its stored
    blocks (BlockColumnSum), the bias gradient of a sparse matrix. No
    atomics: two calls give the same bits. Not differentiable."""
    if not isinstance(sparse, SparseMatrix):
        raise TypeError("column_sum takes a SparseMatrix")
    if sparse.is_transposed():
        raise ValueError("column_sum: not a .t() view")
    _check_dtypes(sparse.data)
    return _column_sum(sparse.data.detach().contiguous(), sparse)


def sdd_act(a: torch.Tensor, b: torch.Tensor, topo: SparseMatrix,
            activation, a_grad_out: Optional[torch.Tensor] = None,
            b_grad_out: Optional[torch.Tensor] = None) -> SparseMatrix:
    """Sparse (topo's blocks) = act(dense @ dense), the activation fused into
    the product (MatmulActivation; "relu", "gelu": the tanh form, "silu").
    The pre-activation is kept for backward, which gates the incoming
    gradient with act' and proceeds as sdd's. Sinks as in sdd."""
    return sdd_act_bias(a, b, topo, activation, a_grad_out, b_grad_out)


def sdd_act_bias(a: torch.Tensor, b: torch.Tensor, topo: SparseMatrix,
                 activation, a_grad_out: Optional[torch.Tensor] = None,
                 b_grad_out: Optional[torch.Tensor] = None, *,
                 bias: Optional[torch.Tensor] = None) -> SparseMatrix:
    """sdd_act with a column bias: act(dense @ dense + bias), `bias` [topo's
    columns] added as sdd_bias adds it (MatmulBiasActivation); the kept
    pre-activation is the biased one. Differentiable in bias too. Without
    `bias` it is sdd_act."""
    return topo.with_data(_SDDAct.apply(
        a, b, topo, _act_code(activation),
        _sink(a_grad_out, a, "sdd_act a_grad_out"),
        _sink(b_grad_out, b, "sdd_act b_grad_out"),
        _column_bias(bias, a, topo, "sdd_act_bias: bias")))


def mlp(x: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor,
        topo: SparseMatrix, activation="gelu",
        w1_grad_out: Optional[torch.Tensor] = None,
        w2_grad_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The expert MLP y = dsd(act(sdd(x, w1, topo)), w2) as one autograd
    function: forward is the fused sdd_act and one dsd; backward computes
    dZ = (dy @ w2^T) * act'(Z) with one MatmulActivationGrad, then dw2 =
    H^T dy, dx = dZ w1^T and dw1 = x^T dZ. Only Z is kept between the passes.
    `w1_grad_out` / `w2_grad_out`: gradient sinks as in sdd / dsd."""
    return mlp_bias(x, w1, w2, topo, activation, w1_grad_out, w2_grad_out)


def mlp_bias(x: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor,
             topo: SparseMatrix, activation="gelu",
             w1_grad_out: Optional[torch.Tensor] = None,
             w2_grad_out: Optional[torch.Tensor] = None, *,
             b1: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mlp with a bias on the hidden matrix: `b1` ([topo's columns], x's
    dtype), Z = x w1 + b1 added in the product's epilogue; db1 =
    column_sum(dZ), cast to b1's dtype. Z is still the only tensor kept
    between the passes besides the operands. Without `b1` it is mlp."""
    return _MLP.apply(x, w1, w2, topo, _act_code(activation),
                      _sink(w1_grad_out, w1, "mlp w1_grad_out"),
                      _sink(w2_grad_out, w2, "mlp w2_grad_out"),
                      _column_bias(b1, x, topo, "mlp_bias: b1"))


def sdd_gated(a: torch.Tensor, b: torch.Tensor, topo: SparseMatrix,
              gate: SparseMatrix, activation,
              a_grad_out: Optional[torch.Tensor] = None,
              b_grad_out: Optional[torch.Tensor] = None) -> SparseMatrix:
    """Sparse (topo's blocks) = (dense @ dense) * act(gate), the gate applied
    in the product's epilogue (MatmulGated). `gate` is a SparseMatrix of
    topo's topology and storage order. Differentiable in a, b and gate.data:
    the product U is kept, backward is one BlockGateGrad giving (dG, dU) and
    then sdd's backward on dU. Sinks as in sdd."""
    return sdd_gated_bias(a, b, topo, gate, activation, a_grad_out, b_grad_out)


def sdd_gated_bias(a: torch.Tensor, b: torch.Tensor, topo: SparseMatrix,
                   gate: SparseMatrix, activation,
                   a_grad_out: Optional[torch.Tensor] = None,
                   b_grad_out: Optional[torch.Tensor] = None, *,
                   bias: Optional[torch.Tensor] = None) -> SparseMatrix:
    """sdd_gated with a column bias: (dense @ dense + bias) * act(gate),
    `bias` [topo's columns] added as sdd_bias adds it (MatmulBiasGated); the
    kept U is the biased one. Differentiable in bias too. Without `bias` it
    is sdd_gated."""
    if not isinstance(gate, SparseMatrix):
        raise TypeError("sdd_gated: gate must be a SparseMatrix")
    if (gate.shape != topo.shape or gate.is_transposed() != topo.is_transposed()
            or gate.data.shape != topo.data.shape):
        raise ValueError("sdd_gated: gate must have topo's shape and blocks")
    return topo.with_data(_SDDGated.apply(
        a, b, gate.data, topo, _act_code(activation),
        _sink(a_grad_out, a, "sdd_gated a_grad_out"),
        _sink(b_grad_out, b, "sdd_gated b_grad_out"),
        _column_bias(bias, a, topo, "sdd_gated_bias: bias")))


def glu_mlp(x: torch.Tensor, w1: torch.Tensor, v1: torch.Tensor,
            w2: torch.Tensor, topo: SparseMatrix, activation="silu",
            w1_grad_out: Optional[torch.Tensor] = None,
            v1_grad_out: Optional[torch.Tensor] = None,
            w2_grad_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The gated expert MLP y = dsd(act(sdd(x, w1)) * sdd(x, v1), w2) as one
    autograd function: forward is Z1 = sdd(x, w1), the fused MatmulGated
    (x, v1, gate Z1, Z2 kept) and one dsd; backward recomputes H for dw2 =
    H^T dy, computes (dZ1, dZ2) with one MatmulGatedGrad of dy @ w2^T (dZ2
    over Z2), then dw1 = x^T dZ1, dv1 = x^T dZ2 and dx = dZ1 w1^T with
    dZ2 v1^T accumulated into it. Only Z1 and Z2 are kept between the passes.
    `*_grad_out`: gradient sinks as in sdd / dsd."""
    return glu_mlp_bias(x, w1, v1, w2, topo, activation, w1_grad_out,
                        v1_grad_out, w2_grad_out)


def glu_mlp_bias(x: torch.Tensor, w1: torch.Tensor, v1: torch.Tensor,
                 w2: torch.Tensor, topo: SparseMatrix, activation="silu",
                 w1_grad_out: Optional[torch.Tensor] = None,
                 v1_grad_out: Optional[torch.Tensor] = None,
                 w2_grad_out: Optional[torch.Tensor] = None, *,
                 b1: Optional[torch.Tensor] = None,
                 bv1: Optional[torch.Tensor] = None) -> torch.Tensor:
    """glu_mlp with biases on its two hidden matrices ([topo's columns], x's
    dtype): `b1` the gate's, Z1 = x w1 + b1, `bv1` the up projection's, Z2 =
    x v1 + bv1, each added in its product's epilogue; db1 = column_sum(dZ1),
    dbv1 = column_sum(dZ2), cast to the bias's dtype. Z1 and Z2 are still the
    only tensors kept besides the operands. Without biases it is glu_mlp."""
    return _GLUMLP.apply(x, w1, v1, w2, topo, _act_code(activation),
                         _sink(w1_grad_out, w1, "glu_mlp w1_grad_out"),
                         _sink(v1_grad_out, v1, "glu_mlp v1_grad_out"),
                         _sink(w2_grad_out, w2, "glu_mlp w2_grad_out"),
                         _column_bias(b1, x, topo, "glu_mlp_bias: b1"),
                         _column_bias(bv1, x, topo, "glu_mlp_bias: bv1"))


def from_dense_mask(x: torch.Tensor, mask) -> SparseMatrix:
    """SparseMatrix holding x's blocks where the [rows/128, cols/128] block
    mask is true (row-major, sorted columns: the reference's mask -> BCSR
    order, matrix_utils.cu:254-289). Test/construction aid."""
    mask = torch.as_tensor(mask, dtype=torch.bool, device=x.device)
    rb, cb = mask.shape
    counts = mask.sum(dim=1, dtype=torch.int32)
    offsets = torch.zeros(rb + 1, dtype=torch.int32, device=x.device)
    offsets[1:] = torch.cumsum(counts, 0)
    r, c = torch.nonzero(mask, as_tuple=True)
    blocks = x.reshape(rb, BLOCK, cb, BLOCK).permute(0, 2, 1, 3)[r, c]
    return SparseMatrix(tuple(x.shape), blocks.contiguous(), offsets,
                        c.to(torch.int16))


def topology_from_mask(mask: torch.Tensor, dtype=torch.float16
                       ) -> SparseMatrix:
    """SparseMatrix (uninitialised block values) whose topology is built
    on the device from a [rows/128, cols/128] block mask."""
    from . import MaskToBcsr
    mask = mask.to(torch.uint8).contiguous()
    rb, cb = mask.shape
    offsets = torch.empty(rb + 1, dtype=torch.int32, device=mask.device)
    cap = torch.empty(max(rb * cb, 1), dtype=torch.int16, device=mask.device)
    MaskToBcsr(mask, offsets, cap)
    nb = int(offsets[-1].item())  # one host sync: the block count sizes data
    data = torch.empty(nb, BLOCK, BLOCK, dtype=dtype, device=mask.device)
    return SparseMatrix((rb * BLOCK, cb * BLOCK), data, offsets,
                        cap[:nb].clone())


def expert_topology(padded_bins: torch.Tensor, blocks_per_expert: int,
                    block_rows: int, dtype=torch.bfloat16) -> SparseMatrix:
    """The dMoE topology (MegaBlocks `topology` op) built on the device:
    block-row r belongs to the expert whose padded bin holds token 128 r and
    owns that expert's `blocks_per_expert` block-columns. No host sync."""
    from . import ExpertTopology
    bins = padded_bins.to(torch.int32).contiguous()
    e = int(bins.numel())
    dev = bins.device
    offsets = torch.empty(block_rows + 1, dtype=torch.int32, device=dev)
    indices = torch.empty(block_rows * blocks_per_expert, dtype=torch.int16,
                          device=dev)
    ExpertTopology(bins, block_rows, blocks_per_expert, offsets, indices)
    data = torch.empty(block_rows * blocks_per_expert, BLOCK, BLOCK,
                       dtype=dtype, device=dev)
    return SparseMatrix((block_rows * BLOCK, e * blocks_per_expert * BLOCK),
                        data, offsets, indices)


# ---- MoE token permutation --------------------------------------------------

def moe_rows_bound(n: int, num_experts: int) -> int:
    """The smallest multiple of 128 that is >= n + 127 * num_experts: the
    worst case of padded_bins[-1] for n assignments (every expert's count one
    past a multiple of 128), so a buffer of that many rows always fits."""
    n, e = int(n), int(num_experts)
    if n < 0 or e < 0:
        raise ValueError("moe_rows_bound: negative n or num_experts")
    return (n + 127 * e + 127) // BLOCK * BLOCK


def _route_rows(rows, n: int, num_experts: int, padded_bins) -> int:
    """Padded rows of a route: the exact size read from the device (one host
    sync) when `rows` is None; else `rows` checked against the bound."""
    if rows is None:
        return int(padded_bins[-1].item()) if num_experts else 0
    if isinstance(rows, bool) or not isinstance(rows, int):
        raise TypeError("rows must be an int or None")
    if rows % BLOCK or rows < moe_rows_bound(n, num_experts):
        raise ValueError(
            f"rows = {rows} must be a multiple of 128 and >= moe_rows_bound"
            f"({n}, {num_experts}) = {moe_rows_bound(n, num_experts)}")
    return rows


@dataclass
class MoeRoute:
    """One routing decision in MegaBlocks' indices_and_padded_bins layout,
    all int32 on the device: `bin_ids` / `indices` the stable ascending sort
    of top_experts.flatten() (indices[i] the assignment t * top_k + k at
    sorted position i), `bins` / `padded_bins` the inclusive cumsums of the
    per-expert counts / of the counts rounded up to multiples of 128,
    `tokens_per_expert` the counts, and `row_of` the padded row of every
    assignment. `rows` is the row count of the padded matrix."""

    indices: torch.Tensor
    bin_ids: torch.Tensor
    bins: torch.Tensor
    padded_bins: torch.Tensor
    tokens_per_expert: torch.Tensor
    row_of: torch.Tensor
    top_k: int
    tokens: int
    rows: int

    @property
    def num_experts(self) -> int:
        return int(self.bins.numel())

    @classmethod
    def from_megablocks(cls, indices, bin_ids, bins, padded_bins, top_k,
                        rows=None) -> "MoeRoute":
        """A route from the tensors MegaBlocks' indices_and_padded_bins
        returns (any integer dtype; converted to int32). `rows` as in
        moe_route."""
        if isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 1:
            raise ValueError(f"top_k must be an int >= 1, not {top_k!r}")
        for name, t in (("indices", indices), ("bin_ids", bin_ids),
                        ("bins", bins), ("padded_bins", padded_bins)):
            if (not isinstance(t, torch.Tensor) or t.dim() != 1
                    or t.dtype.is_floating_point or t.dtype == torch.bool):
                raise TypeError(f"{name} must be a 1-D integer tensor")
        n, e = int(indices.numel()), int(bins.numel())
        if int(bin_ids.numel()) != n or int(padded_bins.numel()) != e:
            raise ValueError("indices / bin_ids and bins / padded_bins must "
                             "pair up in length")
        if n % top_k:
            raise ValueError(f"{n} assignments are not a multiple of top_k = "
                             f"{top_k}")
        if rows is not None:
            _route_rows(rows, n, e, None)
        indices, bin_ids, bins, padded_bins = (
            t.to(torch.int32).contiguous()
            for t in (indices, bin_ids, bins, padded_bins))
        tpe = bins.clone()
        tpe[1:] -= bins[:-1]
        rows = _route_rows(rows, n, e, padded_bins)
        row_of = torch.empty(n, dtype=torch.int32, device=indices.device)
        MoeRowMap(indices, bin_ids, bins, padded_bins, rows, row_of)
        return cls(indices, bin_ids, bins, padded_bins, tpe, row_of, top_k,
                   n // top_k, rows)


def _top_experts(top_experts, num_experts):
    if (not isinstance(top_experts, torch.Tensor)
            or top_experts.dtype.is_floating_point
            or top_experts.dtype == torch.bool):
        raise TypeError("top_experts must be an integer tensor")
    if top_experts.dim() not in (1, 2):
        raise ValueError("top_experts is [tokens, top_k] or [tokens]")
    if (isinstance(num_experts, bool) or not isinstance(num_experts, int)
            or num_experts < 1):
        raise ValueError(f"num_experts must be an int >= 1, not "
                         f"{num_experts!r}")
    tokens = int(top_experts.shape[0])
    top_k = int(top_experts.shape[1]) if top_experts.dim() == 2 else 1
    if top_k < 1:
        raise ValueError("top_experts has no expert per token")
    return tokens, top_k


def moe_route(top_experts: torch.Tensor, num_experts: int,
              rows: Optional[int] = None) -> MoeRoute:
    """The route of a router's `top_experts` ([tokens, top_k] expert ids, or
    [tokens] for top_k = 1). The sort is torch.sort(stable=True); bins,
    padded bins and the row map are built on the device. `rows` None: the
    padded row count is read back once (one host sync; the exact size).
    Explicit `rows`: a multiple of 128 that is >= moe_rows_bound(tokens *
    top_k, num_experts), else ValueError; the route is then built without a
    host sync, and the rows past padded_bins[-1] are zero rows, which
    expert_topology assigns to the last expert."""
    tokens, top_k = _top_experts(top_experts, num_experts)
    n = tokens * top_k
    if rows is not None:
        _route_rows(rows, n, num_experts, None)
    dev = top_experts.device
    bin_ids, indices = torch.sort(top_experts.reshape(-1), stable=True)
    bin_ids = bin_ids.to(torch.int32)
    indices = indices.to(torch.int32)
    bins, tpe, padded_bins = (torch.empty(num_experts, dtype=torch.int32,
                                          device=dev) for _ in range(3))
    MoeBins(bin_ids, num_experts, bins, tpe, padded_bins)
    rows = _route_rows(rows, n, num_experts, padded_bins)
    row_of = torch.empty(n, dtype=torch.int32, device=dev)
    MoeRowMap(indices, bin_ids, bins, padded_bins, rows, row_of)
    return MoeRoute(indices, bin_ids, bins, padded_bins, tpe, row_of, top_k,
                    tokens, rows)


def moe_device_route(top_experts: torch.Tensor, num_experts: int,
                     rows: Optional[int] = None) -> MoeRoute:
    """moe_route with the library's sort: the whole route is one MoeSort (a
    stable counting sort in three launches, num_experts <= 1024;
    sputnik/block/router.h) instead of torch.sort + MoeBins + MoeRowMap. For
    ids in [0, num_experts) every tensor of the route is the same bit for
    bit. The workspace is a per-call temporary from torch's caching
    allocator. `rows` as in moe_route."""
    tokens, top_k = _top_experts(top_experts, num_experts)
    n = tokens * top_k
    if rows is not None:
        _route_rows(rows, n, num_experts, None)
    if num_experts > ROUTER_MAX_EXPERTS:
        raise ValueError(f"moe_device_route: num_experts = {num_experts} "
                         f"passes {ROUTER_MAX_EXPERTS}")
    dev = top_experts.device
    flat = top_experts.reshape(-1).to(torch.int32).contiguous()
    indices, bin_ids, row_of = (torch.empty(n, dtype=torch.int32, device=dev)
                                for _ in range(3))
    bins, tpe, padded_bins = (torch.empty(num_experts, dtype=torch.int32,
                                          device=dev) for _ in range(3))
    chunks = (n + MOE_SORT_CHUNK - 1) // MOE_SORT_CHUNK
    ws = _bt_workspace(chunks * (num_experts + 1) * 4, dev)
    # (rows None: the bound never cuts a row off; the exact size is read
    # back below)
    MoeSort(flat, num_experts,
            moe_rows_bound(n, num_experts) if rows is None else rows,
            indices, bin_ids, bins, tpe, padded_bins, row_of, ws)
    rows = _route_rows(rows, n, num_experts, padded_bins)
    return MoeRoute(indices, bin_ids, bins, padded_bins, tpe, row_of, top_k,
                    tokens, rows)


def _check_route(route, what: str):
    if not isinstance(route, MoeRoute):
        raise TypeError(f"{what}: route must be a MoeRoute")


def _check_rows(t, rows: int, what: str):
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError(f"{what} must be a 2-D tensor")
    _check_dtypes(t)
    if int(t.shape[0]) != rows:
        raise ValueError(f"{what} has {int(t.shape[0])} rows, the route "
                         f"{rows}")


def _check_weights(w, t, route: MoeRoute, what: str):
    if not isinstance(w, torch.Tensor):
        raise TypeError(f"{what}: weights must be a tensor")
    if w.dtype not in (t.dtype, torch.float32):
        raise TypeError(f"{what}: weights are {w.dtype}, expected {t.dtype} "
                        "or torch.float32")
    if (tuple(w.shape) != (route.tokens, route.top_k)
            and tuple(w.shape) != (route.tokens * route.top_k,)):
        raise ValueError(f"{what}: weights have shape {tuple(w.shape)}, "
                         f"expected {(route.tokens, route.top_k)} or flat")


def _gather(x: torch.Tensor, route: MoeRoute, weights) -> torch.Tensor:
    out = torch.empty(route.rows, x.shape[1], dtype=x.dtype, device=x.device)
    PaddedGather(x.contiguous(), route.indices, route.bins, route.padded_bins,
                 out, route.top_k,
                 None if weights is None else weights.contiguous())
    return out


def _scatter(y: torch.Tensor, route: MoeRoute, weights,
             bias=None) -> torch.Tensor:
    out = torch.empty(route.tokens, y.shape[1], dtype=y.dtype, device=y.device)
    w = None if weights is None else weights.contiguous()
    if bias is None:
        PaddedScatter(y.contiguous(), route.row_of, out, route.top_k, w)
    else:
        PaddedScatterBias(y.contiguous(), route.row_of, route.padded_bins,
                          bias, out, route.top_k, w)
    return out


class _PaddedGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, route):
        ctx.route = route
        return _gather(x, route, None)

    @staticmethod
    def backward(ctx, dout):
        return _scatter(dout, ctx.route, None), None  # sum over the copies


class _PaddedScatter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, weights, route, bias=None):
        ctx.route = route
        ctx.save_for_backward(y, weights, bias)
        return _scatter(y, route, weights, bias)

    @staticmethod
    def backward(ctx, dout):
        y, weights, bias = ctx.saved_tensors
        route = ctx.route
        dy = dw = db = None
        dout = dout.contiguous()
        if ctx.needs_input_grad[0]:
            dy = _gather(dout, route, weights)         # w[a] dout[a / top_k]
        if weights is not None and ctx.needs_input_grad[1]:
            dw = torch.empty_like(weights,
                                  memory_format=torch.contiguous_format)
            if bias is None:
                PaddedScatterWeightGrad(dout, y.contiguous(), route.row_of,
                                        dw, route.top_k)
            else:
                PaddedScatterBiasWeightGrad(dout, y.contiguous(),
                                            route.row_of, route.padded_bins,
                                            bias, dw, route.top_k)
        if bias is not None and ctx.needs_input_grad[3]:
            db32 = torch.empty(bias.shape, dtype=torch.float32,
                               device=bias.device)
            PaddedScatterBiasGrad(
                dout, route.indices, route.bins, db32, route.top_k,
                None if weights is None else weights.contiguous())
            db = db32.to(bias.dtype)
        return dy, dw, None, db


def padded_gather(x: torch.Tensor, route: MoeRoute) -> torch.Tensor:
    """x [tokens, hidden] -> [route.rows, hidden] in padded expert order
    (MegaBlocks' padded_gather): row_of[t * top_k + k] holds a copy of x[t],
    every other row is +0. Backward is the unweighted padded_scatter."""
    _check_route(route, "padded_gather")
    _check_rows(x, route.tokens, "padded_gather: x")
    return _PaddedGather.apply(x, route)


def padded_scatter(y: torch.Tensor, route: MoeRoute,
                   weights: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y [route.rows, hidden] -> [tokens, hidden] (MegaBlocks'
    padded_scatter): out[t] = sum_k weights[t, k] * y[row_of[t * top_k + k]],
    summed in fp32 in ascending k and rounded once; a plain sum without
    `weights` ([tokens, top_k] or flat, y's dtype or fp32). Differentiable
    in y (a padded_gather of the incoming gradient with the weights) and in
    weights (PaddedScatterWeightGrad)."""
    return padded_scatter_bias(y, route, weights)


def padded_scatter_bias(y: torch.Tensor, route: MoeRoute,
                        weights: Optional[torch.Tensor] = None, *,
                        bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """padded_scatter with an output bias: `bias` ([num_experts, hidden],
    y's dtype), out[t] = sum_k weights[t, k] * (y[row] + bias[expert of the
    row]), the add in fp32 before the multiply (PaddedScatterBias).
    Differentiable in bias too (PaddedScatterBiasGrad, no atomics, cast to
    its dtype). Without `bias` it is padded_scatter."""
    _check_route(route, "padded_scatter")
    _check_rows(y, route.rows, "padded_scatter: y")
    if weights is not None:
        _check_weights(weights, y, route, "padded_scatter")
    if bias is not None:
        _check_bias(bias, y, (route.num_experts, int(y.shape[1])),
                    "padded_scatter_bias: bias")
        bias = bias.contiguous()
    return _PaddedScatter.apply(y, weights, route, bias)


def _check_moe_biases(x, w1, v1, num_experts: int, biases, what: str):
    """The expert biases (b1, bv1, b2) of a MoE layer, each None or of x's
    dtype and device: b1 / bv1 [w1's columns], b2 [num_experts, d_model]."""
    b1, bv1, b2 = biases
    if bv1 is not None and v1 is None:
        raise ValueError(f"{what}: bv1 is the bias of v1, which is missing")
    for name, t in (("b1", b1), ("bv1", bv1)):
        if t is not None:
            _check_bias(t, x, (int(w1.shape[-1]),), f"{what}: {name}")
    if b2 is not None:
        _check_bias(b2, x, (num_experts, int(x.shape[-1])), f"{what}: b2")


def _moe_args(x, top_experts, expert_weights, w1, w2, v1, num_experts, rows,
              fp8: bool = False):
    """The checks moe_mlp and moe_mlp_fp8 share, up to the route: returns
    (the MoeRoute passed in or None, the expert weights' hidden columns).
    The weights are tensors of x's dtype or, with `fp8`, Fp8Weights (their
    shape is the [k, n] of the weight they hold)."""
    route = top_experts if isinstance(top_experts, MoeRoute) else None
    if route is None:
        tokens, top_k = _top_experts(top_experts, num_experts)
    else:
        tokens, top_k = route.tokens, route.top_k
        if route.num_experts != num_experts:
            raise ValueError(f"moe_mlp: a route over {route.num_experts} "
                             f"experts, num_experts = {num_experts}")
        if rows is not None and rows != route.rows:
            raise ValueError(f"moe_mlp: rows = {rows}, the route has "
                             f"{route.rows}")
    _check_rows(x, tokens, "moe_mlp: x")
    ws = (w1, w2) if v1 is None else (w1, v1, w2)
    if fp8:
        if not all(isinstance(w, Fp8Weight) for w in ws):
            raise TypeError("moe_mlp_fp8: the expert weights are Fp8Weights "
                            "(quantize_weight, Fp8Weight.from_tensors)")
    else:
        _check_dtypes(x, *ws)
    d_model = int(x.shape[1])
    if any(w.dim() != 2 for w in ws):
        raise ValueError("moe_mlp: the expert weights are 2-D")
    hidden = int(w1.shape[1])
    if (int(w1.shape[0]) != d_model or tuple(w2.shape) != (hidden, d_model)
            or (v1 is not None and tuple(v1.shape) != tuple(w1.shape))):
        raise ValueError("moe_mlp: w1 / v1 [d_model, E * ffn], w2 [E * ffn, "
                         "d_model]")
    if hidden == 0 or hidden % (num_experts * BLOCK):
        raise ValueError(f"moe_mlp: {hidden} hidden columns are not "
                         f"{num_experts} experts of a multiple of 128")
    if (not isinstance(expert_weights, torch.Tensor)
            or expert_weights.dtype not in (x.dtype, torch.float32)):
        raise TypeError(f"moe_mlp: expert_weights must be {x.dtype} or "
                        "torch.float32")
    if int(expert_weights.numel()) != tokens * top_k:
        raise ValueError("moe_mlp: one expert weight per (token, k)")
    return route, hidden


def _moe_mlp(x, top_experts, expert_weights, w1, w2, num_experts,
             activation, v1, rows, b1=None, bv1=None, b2=None):
    """moe_mlp's checks and chain; returns the output and the route."""
    route, hidden = _moe_args(x, top_experts, expert_weights, w1, w2, v1,
                              num_experts, rows)
    _check_moe_biases(x, w1, v1, num_experts, (b1, bv1, b2), "moe_mlp")
    act = None if activation is None else _act_code(activation)
    if route is None:
        route = moe_route(top_experts, num_experts, rows)
    xp = padded_gather(x, route)
    topo = expert_topology(route.padded_bins, hidden // num_experts // BLOCK,
                           route.rows // BLOCK, dtype=x.dtype)
    if v1 is None:
        y = mlp_bias(xp, w1, w2, topo, "gelu" if act is None else act, b1=b1)
    else:
        y = glu_mlp_bias(xp, w1, v1, w2, topo,
                         "silu" if act is None else act, b1=b1, bv1=bv1)
    return padded_scatter_bias(y, route, expert_weights, bias=b2), route


def moe_mlp(x: torch.Tensor, top_experts: torch.Tensor,
            expert_weights: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor,
            num_experts: int, activation=None,
            v1: Optional[torch.Tensor] = None,
            rows: Optional[int] = None) -> torch.Tensor:
    """A dropless MoE layer behind its router: moe_route(top_experts) ->
    padded_gather(x) -> expert_topology -> mlp (glu_mlp when `v1` is given)
    -> padded_scatter with `expert_weights`. x [tokens, d_model]; w1 (and
    v1) [d_model, num_experts * ffn], w2 [num_experts * ffn, d_model], ffn a
    multiple of 128, expert e owning columns / rows [e * ffn, (e + 1) * ffn).
    `activation` None: the MLP's default ("gelu" for mlp, "silu" for
    glu_mlp). `rows` as in moe_route (None: one host sync for the exact
    padded size; moe_rows_bound(tokens * top_k, num_experts) or more: none).
    `top_experts` may also be a MoeRoute built beforehand (moe_route,
    moe_device_route, MoeRoute.from_megablocks): the layer then uses it as
    it is, and `rows`, when given, must be its row count. Differentiable in
    x, expert_weights, w1, v1 and w2."""
    return _moe_mlp(x, top_experts, expert_weights, w1, w2, num_experts,
                    activation, v1, rows)[0]


def moe_mlp_bias(x: torch.Tensor, top_experts: torch.Tensor,
                 expert_weights: torch.Tensor, w1: torch.Tensor,
                 w2: torch.Tensor, num_experts: int, activation=None,
                 v1: Optional[torch.Tensor] = None,
                 rows: Optional[int] = None, *,
                 b1: Optional[torch.Tensor] = None,
                 bv1: Optional[torch.Tensor] = None,
                 b2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """moe_mlp with expert biases, all of x's dtype: `b1` [num_experts * ffn]
    on x w1 (the gate of a GLU), `bv1` the same on x v1, `b2` [num_experts,
    d_model] on the expert's output, added before the router weight
    multiplies it (mlp_bias / glu_mlp_bias, padded_scatter_bias).
    Differentiable in each. Without biases it is moe_mlp."""
    return _moe_mlp(x, top_experts, expert_weights, w1, w2, num_experts,
                    activation, v1, rows, b1, bv1, b2)[0]


# ---- FP8 (e4m3) expert products ----------------------------------------------

@dataclass
class Fp8Weight:
    """A weight [k, n] quantised for the fp8 products (sputnik/block/fp8.h):
    `q` torch.float8_e4m3fn [n, k] (k-contiguous) and `scales` fp32 [k / 128,
    n / 128], one per 128 x 128 block, value = float(q) * scale. `shape` is
    the (k, n) of the weight it stands for."""

    q: torch.Tensor
    scales: torch.Tensor
    k: int
    n: int

    @property
    def shape(self):
        return (self.k, self.n)

    def dim(self) -> int:
        return 2

    @classmethod
    def from_tensors(cls, q: torch.Tensor, scales: torch.Tensor
                     ) -> "Fp8Weight":
        """Checkpoint data as it is: `q` [n, k] (out features x in features)
        of torch.float8_e4m3fn, or of torch.uint8 holding those bytes, and
        `scales` fp32 [k / 128, n / 128]. Nothing is copied unless a tensor
        is not contiguous."""
        if not isinstance(q, torch.Tensor) or q.dim() != 2:
            raise ValueError("Fp8Weight: q is a 2-D tensor [n, k]")
        if q.dtype == torch.uint8:
            q = q.view(torch.float8_e4m3fn)
        if q.dtype != torch.float8_e4m3fn:
            raise TypeError(f"Fp8Weight: q is {q.dtype}, expected "
                            "torch.float8_e4m3fn (or its bytes as uint8)")
        n, k = int(q.shape[0]), int(q.shape[1])
        if n % BLOCK or k % BLOCK:
            raise ValueError(f"Fp8Weight: [n, k] = [{n}, {k}] is not a "
                             "multiple of 128")
        if (not isinstance(scales, torch.Tensor)
                or scales.dtype != torch.float32):
            raise TypeError("Fp8Weight: scales must be a torch.float32 tensor")
        if tuple(scales.shape) != (k // BLOCK, n // BLOCK):
            raise ValueError(f"Fp8Weight: scales have shape "
                             f"{tuple(scales.shape)}, expected "
                             f"{(k // BLOCK, n // BLOCK)} ([k / 128, n / 128])")
        return cls(q.contiguous(), scales.contiguous(), k, n)

    def t(self) -> "Fp8Weight":
        """The Fp8Weight of the transposed weight [n, k]: an exact byte
        transpose, bit for bit quantize_weight of the transposed 16-bit
        weight. The backward layout of a weight that exists only as fp8."""
        qt = torch.empty(self.k, self.n, dtype=torch.float8_e4m3fn,
                         device=self.q.device)
        st = torch.empty(self.n // BLOCK, self.k // BLOCK,
                         dtype=torch.float32, device=self.q.device)
        TransposeWeightFp8(self.q, self.scales, qt, st)
        return Fp8Weight(qt, st, self.n, self.k)


class Fp8SparseMatrix(SparseMatrix):
    """A SparseMatrix whose block values are e4m3 bytes, with `scales` fp32
    [nnz_blocks * 128]: one per row of each stored block, in storage order
    (quantize_sparse). The operand of dsd_fp8."""

    def __init__(self, topo: SparseMatrix, q: torch.Tensor,
                 scales: torch.Tensor):
        m = topo._meta
        super().__init__((m.rows, m.cols), q, m.offsets, m.indices, _meta=m)
        self.scales = scales


def _no_grad(what: str, *ts):
    if torch.is_grad_enabled() and any(
            isinstance(t, torch.Tensor) and t.requires_grad for t in ts):
        raise ValueError(f"{what} is forward only: an input requires grad "
                         "and no gradient would reach it (use torch.no_grad() "
                         "or detach())")


def quantize_rows(x: torch.Tensor, pow2: bool = False
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(q, scales) of x [rows, cols] (fp16 / bf16, cols a multiple of 128):
    q torch.float8_e4m3fn of x's shape, scales fp32 [rows, cols / 128], one
    per 1 x 128 tile, x ~ float(q) * scale. scale = max(amax / 448, 2^-126)
    or, with `pow2`, the smallest power of two that fits (dequantisation is
    then exact); sputnik/block/fp8.h has the format. Forward only."""
    _check_dtypes(x)
    _no_grad("quantize_rows", x)
    if x.dim() != 2 or int(x.shape[1]) % BLOCK:
        raise ValueError("quantize_rows: x is [rows, a multiple of 128]")
    x = x.contiguous()
    q = torch.empty(x.shape, dtype=torch.float8_e4m3fn, device=x.device)
    scales = torch.empty(x.shape[0], x.shape[1] // BLOCK,
                         dtype=torch.float32, device=x.device)
    QuantizeRows(x, q, scales, pow2)
    return q, scales


def quantize_sparse(sparse: SparseMatrix, activation=None,
                    gate: Optional[SparseMatrix] = None,
                    pow2: bool = False) -> Fp8SparseMatrix:
    """The block values of `sparse` (fp16 / bf16) quantised row by row of
    each stored block, as the matrix [nnz_blocks * 128, 128]. With
    `activation` alone the values of act(sparse) are quantised, with `gate`
    (same topology and dtype) those of sparse * act(gate), each evaluated as
    sdd_act / sdd_gated evaluate it, so the result is the quantisation of the
    hidden matrix the 16-bit MLP stores, which is never written here. Forward
    only."""
    if not isinstance(sparse, SparseMatrix) or sparse.is_transposed():
        raise TypeError("quantize_sparse takes a SparseMatrix (not a .t() "
                        "view)")
    _check_dtypes(sparse.data)
    _no_grad("quantize_sparse", sparse.data,
             None if gate is None else gate.data)
    g = None
    if gate is not None:
        if (not isinstance(gate, SparseMatrix)
                or gate._meta is not sparse._meta or gate.is_transposed()
                or gate.dtype != sparse.dtype):
            raise ValueError("quantize_sparse: gate must share sparse's "
                             "topology and dtype")
        if activation is None:
            raise ValueError("quantize_sparse: a gate needs its activation")
        g = gate.data.contiguous().view(-1, BLOCK)
    nb = sparse.nnz_blocks
    x = sparse.data.contiguous().view(nb * BLOCK, BLOCK)
    q = torch.empty(nb, BLOCK, BLOCK, dtype=torch.float8_e4m3fn,
                    device=x.device)
    scales = torch.empty(nb * BLOCK, dtype=torch.float32, device=x.device)
    QuantizeRows(x, q.view(nb * BLOCK, BLOCK), scales.view(nb * BLOCK, 1),
                 pow2, None if activation is None else _act_code(activation),
                 g)
    return Fp8SparseMatrix(sparse, q, scales)


def quantize_weight(w: torch.Tensor, transpose: bool = False,
                    pow2: bool = False) -> Fp8Weight:
    """The Fp8Weight of w [k, n] (fp16 / bf16, both multiples of 128); with
    `transpose` the tensor passed is w^T, [n, k], as checkpoints store a
    linear layer. One scale per 128 x 128 block. Runs once, at load time."""
    _check_dtypes(w)
    _no_grad("quantize_weight", w)
    if w.dim() != 2 or int(w.shape[0]) % BLOCK or int(w.shape[1]) % BLOCK:
        raise ValueError("quantize_weight: w is 2-D with multiples of 128")
    w = w.contiguous()
    k, n = (int(w.shape[1]), int(w.shape[0])) if transpose else (
        int(w.shape[0]), int(w.shape[1]))
    q = torch.empty(n, k, dtype=torch.float8_e4m3fn, device=w.device)
    scales = torch.empty(k // BLOCK, n // BLOCK, dtype=torch.float32,
                         device=w.device)
    QuantizeWeight(w, q, scales, transpose, pow2)
    return Fp8Weight(q, scales, k, n)


def _out_dtype(out_dtype, what: str):
    if out_dtype not in (torch.float16, torch.bfloat16):
        raise TypeError(f"{what}: out_dtype must be torch.float16 or "
                        "torch.bfloat16")


def _accumulate(accumulate, what: str) -> str:
    """"fp32" or "fast" (sputnik/block/fp8.h, Fp8Accumulate); raises before
    any GPU call."""
    if not isinstance(accumulate, str) or accumulate not in FP8_ACCUMULATE:
        raise ValueError(f"{what}: accumulate must be 'fp32' or 'fast', not "
                         f"{accumulate!r}")
    return accumulate


def sdd_fp8(xq: torch.Tensor, xs: torch.Tensor, w: Fp8Weight,
            topo: SparseMatrix, out_dtype=torch.bfloat16,
            accumulate: str = "fp32") -> SparseMatrix:
    """(xq . w) at topo's nonzero blocks, the product in fp8: xq / xs from
    quantize_rows ([m, k] and [m, k / 128]), w an Fp8Weight of [k, n], topo
    [m, n]. Per 128-wide k-block the e4m3 products are summed by the matrix
    cores in fp32 and added as (xs * w.scales) * sum; the block values are
    rounded once to `out_dtype`. Bitwise reproducible. Forward only.
    `accumulate="fast"` opts into the scaled e4m3 MFMA for the k-block sums:
    twice the matrix-core rate, the sums at that instruction's limited
    precision (fp8.h has the bound), still bitwise reproducible."""
    _accumulate(accumulate, "sdd_fp8")
    if not isinstance(w, Fp8Weight):
        raise TypeError("sdd_fp8: w must be an Fp8Weight")
    if not isinstance(topo, SparseMatrix) or topo.is_transposed():
        raise TypeError("sdd_fp8: topo must be a SparseMatrix (not a .t() "
                        "view)")
    _out_dtype(out_dtype, "sdd_fp8")
    _no_grad("sdd_fp8", xs)
    if (not isinstance(xq, torch.Tensor) or xq.dim() != 2
            or (int(xq.shape[0]), w.n) != tuple(topo.shape)
            or int(xq.shape[1]) != w.k):
        raise ValueError(f"sdd_fp8 shapes {tuple(getattr(xq, 'shape', ()))} "
                         f"x {w.shape} -> {topo.shape}")
    data = torch.empty(topo.nnz_blocks, BLOCK, BLOCK, dtype=out_dtype,
                       device=xq.device)
    topo._meta.ensure_row_indices(data)
    SddFp8(xq, xs, w.q, w.scales, topo._meta.descriptor(data),
           accumulate=accumulate)
    return topo.with_data(data)


def dsd_fp8(sq: Fp8SparseMatrix, w: Fp8Weight, out_dtype=torch.bfloat16,
            accumulate: str = "fp32") -> torch.Tensor:
    """sq . w as a dense [m, n] tensor of `out_dtype`, the product in fp8:
    sq from quantize_sparse ([m, k]), w an Fp8Weight of [k, n]. Arithmetic as
    sdd_fp8, over the stored blocks of each block row in storage order; a
    block row without blocks gives +0 rows. Forward only. `accumulate` as
    sdd_fp8."""
    _accumulate(accumulate, "dsd_fp8")
    if not isinstance(sq, Fp8SparseMatrix):
        raise TypeError("dsd_fp8: sq must come from quantize_sparse")
    if not isinstance(w, Fp8Weight):
        raise TypeError("dsd_fp8: w must be an Fp8Weight")
    _out_dtype(out_dtype, "dsd_fp8")
    if sq.shape[1] != w.k:
        raise ValueError(f"dsd_fp8 shapes {sq.shape} x {w.shape}")
    out = torch.empty(sq.shape[0], w.n, dtype=out_dtype, device=sq.device)
    DsdFp8(sq._descriptor(), sq.scales, w.q, w.scales,
           Matrix(out.shape[0], out.shape[1], out), accumulate=accumulate)
    return out


def moe_mlp_fp8(x: torch.Tensor, top_experts: torch.Tensor,
                expert_weights: torch.Tensor, w1q: Fp8Weight, w2q: Fp8Weight,
                num_experts: int, activation=None,
                v1q: Optional[Fp8Weight] = None,
                rows: Optional[int] = None,
                accumulate: str = "fp32") -> torch.Tensor:
    """moe_mlp with the expert products in fp8 (e4m3 elements, fp32 scales
    per 1 x 128 activation tile and per 128 x 128 weight block, the recipe of
    DeepSeek-V3 checkpoints; sputnik/block/fp8.h): padded_gather ->
    quantize_rows -> sdd_fp8 with `w1q` (and with `v1q` for a GLU) ->
    quantize_sparse with the activation (or the gate) -> dsd_fp8 with `w2q`
    -> padded_scatter. The two (three) expert products run in fp8 with fp32
    accumulation; the gather, the activation, the scatter with
    `expert_weights` and the router stay in x's 16-bit dtype, which is also
    the products' output type. `w1q` / `v1q` stand for [d_model,
    num_experts * ffn] and `w2q` for [num_experts * ffn, d_model]
    (quantize_weight, Fp8Weight.from_tensors). Arguments, defaults and route
    handling are moe_mlp's; there are no biases. Forward only: the output
    carries no gradient, and a tensor that requires grad while grad mode is
    on is a ValueError. `accumulate` ("fp32", the default, or "fast") is
    passed to the two (three) products; everything else is unchanged."""
    _accumulate(accumulate, "moe_mlp_fp8")
    _no_grad("moe_mlp_fp8", x, expert_weights)
    route, hidden = _moe_args(x, top_experts, expert_weights, w1q, w2q, v1q,
                              num_experts, rows, fp8=True)
    act = None if activation is None else _act_code(activation)
    if route is None:
        route = moe_route(top_experts, num_experts, rows)
    xp = padded_gather(x, route)
    topo = expert_topology(route.padded_bins, hidden // num_experts // BLOCK,
                           route.rows // BLOCK, dtype=x.dtype)
    xq, xs = quantize_rows(xp)
    g = sdd_fp8(xq, xs, w1q, topo, x.dtype, accumulate)
    if v1q is None:
        hq = quantize_sparse(g, "gelu" if act is None else act)
    else:
        u = sdd_fp8(xq, xs, v1q, topo, x.dtype, accumulate)
        hq = quantize_sparse(u, "silu" if act is None else act, gate=g)
    return padded_scatter(dsd_fp8(hq, w2q, x.dtype, accumulate), route,
                          expert_weights)


# ---- FP8 gradients (sputnik/block/fp8.h, "Gradients") ------------------------

def quantize_tiles(x: torch.Tensor, rows: bool = True, cols: bool = True,
                   pow2: bool = False):
    """(q, scales, qt, scales_t) of x [rows, cols] (fp16 / bf16, both
    multiples of 128), read once: q / scales as quantize_rows, bit for bit;
    qt torch.float8_e4m3fn [cols, rows] and scales_t fp32 [rows / 128, cols]
    with one scale per 128 x 1 column tile, the dense operand of
    dsd_fp8_wgrad. A pair that is not asked for is (None, None)."""
    _check_dtypes(x)
    _no_grad("quantize_tiles", x)
    if x.dim() != 2 or int(x.shape[0]) % BLOCK or int(x.shape[1]) % BLOCK:
        raise ValueError("quantize_tiles: x is 2-D with multiples of 128")
    if not (rows or cols):
        raise ValueError("quantize_tiles: no output asked for")
    x = x.contiguous()
    m, n = int(x.shape[0]), int(x.shape[1])
    q = s = qt = st = None
    if rows:
        q = torch.empty(m, n, dtype=torch.float8_e4m3fn, device=x.device)
        s = torch.empty(m, n // BLOCK, dtype=torch.float32, device=x.device)
    if cols:
        qt = torch.empty(n, m, dtype=torch.float8_e4m3fn, device=x.device)
        st = torch.empty(m // BLOCK, n, dtype=torch.float32, device=x.device)
    QuantizeTiles(x, q, s, qt, st, pow2)
    return q, s, qt, st


def _quantize_blocks(sparse: SparseMatrix, stage, act, z, rows: bool,
                     cols: bool, pow2: bool):
    """QuantizeBlocks over sparse's block values: (the Fp8SparseMatrix of
    sparse's topology or None, the Fp8SparseMatrix of the transposed
    topology or None)."""
    meta, nb = sparse._meta, sparse.nnz_blocks
    data = sparse.data.contiguous()
    dev = data.device
    q = s = qt = st = None
    if rows:
        q = torch.empty(nb, BLOCK, BLOCK, dtype=torch.float8_e4m3fn,
                        device=dev)
        s = torch.empty(nb * BLOCK, dtype=torch.float32, device=dev)
    if cols:
        meta.ensure_transposed(data)
        qt = torch.empty(nb, BLOCK, BLOCK, dtype=torch.float8_e4m3fn,
                         device=dev)
        st = torch.empty(nb * BLOCK, dtype=torch.float32, device=dev)
    if nb:
        QuantizeBlocks(meta.descriptor(data), q, s, qt, st, stage, act,
                       None if z is None else z.contiguous(), pow2)
    by_rows = Fp8SparseMatrix(sparse, q, s) if rows else None
    by_cols = None
    if cols:
        by_cols = Fp8SparseMatrix(
            SparseMatrix((meta.cols, meta.rows), qt, meta.offsets_t,
                         meta.indices_t), qt, st)
    return by_rows, by_cols


def quantize_sparse_t(sparse: SparseMatrix, activation=None,
                      z: Optional[SparseMatrix] = None,
                      pow2: bool = False) -> Fp8SparseMatrix:
    """The Fp8SparseMatrix of sparse^T, the sparse operand of dsd_fp8_wgrad:
    its blocks are sparse's, transposed and in the transposed order, each
    with 128 per-row scales, one per column of the source block (a 128 x 1
    tile of sparse). With `activation` alone act(sparse) is quantised, as
    quantize_sparse does it; with `z` (same topology and dtype) sparse *
    act'(z), as sdd_act's gradient evaluates it, rounded to sparse's dtype
    first."""
    if not isinstance(sparse, SparseMatrix) or sparse.is_transposed():
        raise TypeError("quantize_sparse_t takes a SparseMatrix (not a .t() "
                        "view)")
    _check_dtypes(sparse.data)
    _no_grad("quantize_sparse_t", sparse.data, None if z is None else z.data)
    stage = None
    if z is not None:
        if (not isinstance(z, SparseMatrix) or z._meta is not sparse._meta
                or z.is_transposed() or z.dtype != sparse.dtype):
            raise ValueError("quantize_sparse_t: z must share sparse's "
                             "topology and dtype")
        if activation is None:
            raise ValueError("quantize_sparse_t: z needs its activation")
        stage = "act_grad"
    elif activation is not None:
        stage = "act"
    act = None if activation is None else _act_code(activation)
    return _quantize_blocks(sparse, stage, act,
                            None if z is None else z.data, False, True,
                            pow2)[1]


def dsd_fp8_wgrad(st: Fp8SparseMatrix, bqt: torch.Tensor, bst: torch.Tensor,
                  out: Optional[torch.Tensor] = None, add: bool = False,
                  out_dtype=torch.bfloat16,
                  accumulate: str = "fp32") -> torch.Tensor:
    """st . B as a dense [m, n] tensor, the weight-gradient product in fp8:
    st from quantize_sparse_t ([m, k], k the token dimension), B [k, n] given
    as quantize_tiles' column pair bqt [n, k], bst [k / 128, n]. Per k-block
    in st's storage order acc = fma(st.scales[row] * bst[kb, col], P, acc);
    `accumulate` as sdd_fp8. Writes `out` (contiguous [m, n], fp16 / bf16 /
    fp32) or a new tensor of `out_dtype` (the same three); with `add`, out =
    round(acc + out), rounded once, and rows that meet no block of st are
    left untouched. Bitwise reproducible."""
    _accumulate(accumulate, "dsd_fp8_wgrad")
    if not isinstance(st, Fp8SparseMatrix):
        raise TypeError("dsd_fp8_wgrad: st must come from quantize_sparse_t")
    if not isinstance(bqt, torch.Tensor) or bqt.dim() != 2:
        raise TypeError("dsd_fp8_wgrad: bqt is quantize_tiles' qt")
    m, n = st.shape[0], int(bqt.shape[0])
    if st.shape[1] != int(bqt.shape[1]):
        raise ValueError(f"dsd_fp8_wgrad shapes {st.shape} x "
                         f"{(int(bqt.shape[1]), n)}")
    if out is None:
        if add:
            raise ValueError("dsd_fp8_wgrad: add needs `out`")
        if out_dtype not in (torch.float16, torch.bfloat16, torch.float32):
            raise TypeError("dsd_fp8_wgrad: out_dtype must be torch.float16, "
                            "torch.bfloat16 or torch.float32")
        out = torch.empty(m, n, dtype=out_dtype, device=bqt.device)
    else:
        if (not isinstance(out, torch.Tensor) or tuple(out.shape) != (m, n)
                or not out.is_contiguous()):
            raise ValueError(f"dsd_fp8_wgrad: out must be a contiguous "
                             f"{(m, n)} tensor")
        if out.dtype not in (torch.float16, torch.bfloat16, torch.float32):
            raise TypeError("dsd_fp8_wgrad: out must be fp16, bf16 or fp32")
    DsdFp8Wgrad(st._descriptor(), st.scales, bqt, bst, Matrix(m, n, out),
                add=add, accumulate=accumulate)
    return out


class _MLPFp8(torch.autograd.Function):
    """y = dsd_fp8(quantize_sparse(sdd_fp8(x, w1t^T), act), w2) and the
    backward pass of fp8.h's table. Keeps Z, the column quantisation of X
    (bytes, not the 16-bit X) and the backward layouts of the two weights."""

    @staticmethod
    def forward(ctx, x, w1t, w2, topo, act, accumulate, pow2, w1_sink,
                w2_sink):
        need_x, need_w1, need_w2 = ctx.needs_input_grad[:3]
        need_w1 = need_w1 or w1_sink is not None
        need_w2 = need_w2 or w2_sink is not None
        ctx.topo, ctx.act, ctx.mode, ctx.pow2 = topo, act, accumulate, pow2
        ctx.w1_sink, ctx.w2_sink = w1_sink, w2_sink
        ctx.need = (need_x, need_w1, need_w2)
        w1q = quantize_weight(w1t, transpose=True, pow2=pow2)   # [h, F]
        w2q = quantize_weight(w2, pow2=pow2)                    # [F, h]
        xq, xs, xqt, xst = quantize_tiles(x, cols=need_w1, pow2=pow2)
        z = sdd_fp8(xq, xs, w1q, topo, x.dtype, accumulate)
        y = dsd_fp8(quantize_sparse(z, act, pow2=pow2), w2q, x.dtype,
                    accumulate)
        if any(ctx.need):
            # (dH = dY W2^T and dX = dZ W1t take the transposed layouts)
            ctx.w2q_t = w2q.t() if need_x or need_w1 else None
            ctx.w1q_t = w1q.t() if need_x else None
            ctx.save_for_backward(z.data, xqt, xst)
        return y

    @staticmethod
    def backward(ctx, dy):
        z_data, xqt, xst = ctx.saved_tensors
        need_x, need_w1, need_w2 = ctx.need
        topo, act, mode, pow2 = ctx.topo, ctx.act, ctx.mode, ctx.pow2
        z = topo.with_data(z_data)
        dt = z_data.dtype
        dx = dw1 = dw2 = None
        need_dz = need_x or need_w1
        dyq, dys, dyqt, dyst = quantize_tiles(dy, rows=need_dz, cols=need_w2,
                                              pow2=pow2)
        if need_w2:                                   # H^T dY
            ht = _quantize_blocks(z, "act", act, None, False, True, pow2)[1]
            if ctx.w2_sink is not None:
                dsd_fp8_wgrad(ht, dyqt, dyst, ctx.w2_sink, True,
                              accumulate=mode)
            else:
                dw2 = dsd_fp8_wgrad(ht, dyqt, dyst, out_dtype=dt,
                                    accumulate=mode)
            del ht
        if need_dz:
            dh = sdd_fp8(dyq, dys, ctx.w2q_t, topo, dt, mode)   # dY W2^T
            # dZ = dH * act'(Z), quantised along both axes in one pass
            dzq, dzt = _quantize_blocks(dh, "act_grad", act, z_data, need_x,
                                        need_w1, pow2)
            if need_x:
                dx = dsd_fp8(dzq, ctx.w1q_t, dt, mode)          # dZ W1t
            if ctx.w1_sink is not None:                         # dZ^T X
                dsd_fp8_wgrad(dzt, xqt, xst, ctx.w1_sink, True,
                              accumulate=mode)
            elif need_w1:
                dw1 = dsd_fp8_wgrad(dzt, xqt, xst, out_dtype=dt,
                                    accumulate=mode)
        return dx, dw1, dw2, None, None, None, None, None, None


def mlp_fp8(x: torch.Tensor, w1t: torch.Tensor, w2: torch.Tensor,
            topo: SparseMatrix, activation="gelu", accumulate: str = "fp32",
            pow2: bool = False, w1t_grad_out: Optional[torch.Tensor] = None,
            w2_grad_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The expert MLP with its three products in fp8, forward and backward:
    y = act(x w1t^T at topo's blocks) w2 over 16-bit x [T, h], w1t [F, h] and
    w2 [F, h] (MegaBlocks' orientation), topo [T, F]. Forward quantises the
    weights (quantize_weight, and Fp8Weight.t() for the backward layouts)
    and runs quantize_rows -> sdd_fp8 -> quantize_sparse(activation) ->
    dsd_fp8, bit for bit. Backward (sputnik/block/fp8.h, "Gradients"): dH =
    dY W2^T by sdd_fp8, dZ = dH * act'(Z) fused into the quantiser, dX = dZ
    W1t by dsd_fp8, and dW2 = H^T dY, dW1t = dZ^T X by dsd_fp8_wgrad with
    both operands scaled per 128 tokens x 1 column. The gradients are
    straight-through: taken with respect to the 16-bit inputs, in their
    dtype. A sink (`w1t_grad_out`, `w2_grad_out`: contiguous [F, h], x's
    dtype or fp32) receives sink += gradient, rounded once, in place of a
    returned gradient. What needs_input_grad does not ask for is skipped.
    There are no biases and no GLU form."""
    _accumulate(accumulate, "mlp_fp8")
    _check_dtypes(x, w1t, w2)
    if not isinstance(topo, SparseMatrix) or topo.is_transposed():
        raise TypeError("mlp_fp8: topo must be a SparseMatrix (not a .t() "
                        "view)")
    if (x.dim() != 2 or w1t.dim() != 2 or tuple(w1t.shape) != tuple(w2.shape)
            or tuple(topo.shape) != (int(x.shape[0]), int(w1t.shape[0]))
            or int(w1t.shape[1]) != int(x.shape[1])
            or int(x.shape[1]) % BLOCK):
        raise ValueError("mlp_fp8: x [T, h], w1t and w2 [F, h], topo [T, F], "
                         "all multiples of 128")
    for sink, what in ((w1t_grad_out, "w1t_grad_out"),
                       (w2_grad_out, "w2_grad_out")):
        if sink is not None:
            _check_sink(sink, int(w2.shape[0]), int(w2.shape[1]), x.dtype,
                        f"mlp_fp8: {what}")
    return _MLPFp8.apply(x.contiguous(), w1t.contiguous(), w2.contiguous(),
                         topo, _act_code(activation), accumulate, bool(pow2),
                         w1t_grad_out, w2_grad_out)


def moe_mlp_fp8_train(x: torch.Tensor, top_experts: torch.Tensor,
                      expert_weights: torch.Tensor, w1t: torch.Tensor,
                      w2: torch.Tensor, num_experts: int, activation=None,
                      rows: Optional[int] = None, accumulate: str = "fp32",
                      pow2: bool = False,
                      w1t_grad_out: Optional[torch.Tensor] = None,
                      w2_grad_out: Optional[torch.Tensor] = None
                      ) -> torch.Tensor:
    """moe_mlp with the expert products in fp8 and gradients: padded_gather
    -> mlp_fp8 -> padded_scatter, the permutation with its existing
    gradients. w1t and w2 are 16-bit [num_experts * ffn, d_model]; the other
    arguments are moe_mlp's (activation None: "gelu"). Differentiable in x,
    expert_weights, w1t and w2."""
    _accumulate(accumulate, "moe_mlp_fp8_train")
    if not isinstance(w1t, torch.Tensor) or w1t.dim() != 2:
        raise ValueError("moe_mlp_fp8_train: w1t is [E * ffn, d_model]")
    route, hidden = _moe_args(x, top_experts, expert_weights, w1t.t(), w2,
                              None, num_experts, rows)
    if route is None:
        route = moe_route(top_experts, num_experts, rows)
    xp = padded_gather(x, route)
    topo = expert_topology(route.padded_bins, hidden // num_experts // BLOCK,
                           route.rows // BLOCK, dtype=x.dtype)
    y = mlp_fp8(xp, w1t, w2, topo, "gelu" if activation is None else
                activation, accumulate, pow2, w1t_grad_out, w2_grad_out)
    return padded_scatter(y, route, expert_weights)


# ---- MoE router -------------------------------------------------------------

def _router_forward(ctx, logits, top_k, normalize, dtype):
    """What _Router and _RouterAux begin with: (contiguous logits, top,
    weights), the outputs allocated, and the context set up for
    _router_backward (top carries no gradient, absent gradients stay None)."""
    logits = logits.contiguous()
    tokens = logits.shape[0]
    top = torch.empty(tokens, top_k, dtype=torch.int32, device=logits.device)
    weights = torch.empty(tokens, top_k, dtype=dtype, device=logits.device)
    ctx.save_for_backward(logits, top)
    ctx.normalize = normalize
    ctx.dtype = dtype
    ctx.set_materialize_grads(False)
    ctx.mark_non_differentiable(top)
    return logits, top, weights


def _router_backward(ctx, dweights, *others):
    """(logits, top, dweights, dlogits) for the gradient call, an absent
    dweights as zeros; None when every incoming gradient is absent."""
    if dweights is None and all(g is None for g in others):
        return None
    logits, top = ctx.saved_tensors
    if dweights is None:
        dweights = torch.zeros(top.shape, dtype=ctx.dtype,
                               device=logits.device)
    return logits, top, dweights.contiguous(), torch.empty_like(logits)


def _contiguous(g):
    return None if g is None else g.contiguous()


class _Router(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, top_k, normalize, dtype, return_scores):
        logits, top, weights = _router_forward(ctx, logits, top_k, normalize,
                                               dtype)
        scores = (torch.empty(logits.shape, dtype=dtype, device=logits.device)
                  if return_scores else None)
        RouterTopK(logits, top, weights, normalize, scores)
        return (weights, top, scores) if return_scores else (weights, top)

    @staticmethod
    def backward(ctx, dweights, _dtop, dscores=None):
        args = _router_backward(ctx, dweights, dscores)
        if args is None:
            return None, None, None, None, None
        logits, top, dweights, dlogits = args
        RouterTopKGrad(logits, top, dweights, dlogits, ctx.normalize,
                       _contiguous(dscores))
        return dlogits, None, None, None, None


def _router_args(logits, top_k, weights_dtype, what: str):
    """The checks moe_router and moe_router_aux share; returns the dtype of
    the weights."""
    if (not isinstance(logits, torch.Tensor) or logits.dtype not in
            (torch.float16, torch.bfloat16, torch.float32)):
        raise TypeError(f"{what}: logits must be an fp16, bf16 or fp32 "
                        "tensor")
    if logits.dim() != 2:
        raise ValueError(f"{what}: logits are [tokens, num_experts]")
    e = int(logits.shape[1])
    if not 1 <= e <= ROUTER_MAX_EXPERTS:
        raise ValueError(f"{what}: {e} experts, outside [1, "
                         f"{ROUTER_MAX_EXPERTS}]")
    if (isinstance(top_k, bool) or not isinstance(top_k, int)
            or not 1 <= top_k <= min(e, ROUTER_MAX_TOP_K)):
        raise ValueError(f"{what}: top_k must be an int in [1, min({e}, "
                         f"{ROUTER_MAX_TOP_K})], not {top_k!r}")
    if weights_dtype is None:
        weights_dtype = logits.dtype
    elif weights_dtype not in (logits.dtype, torch.float32):
        raise TypeError(f"{what}: weights_dtype must be {logits.dtype} "
                        "or torch.float32")
    return weights_dtype


def moe_router(logits: torch.Tensor, top_k: int, normalize: bool = False,
               weights_dtype=None, return_scores: bool = False):
    """The router's choice from its logits [tokens, E] (fp16, bf16 or fp32):
    (expert_weights [tokens, top_k], top_experts int32 [tokens, top_k]) and,
    with `return_scores`, scores [tokens, E] (the softmax, for a
    load-balancing loss). The picks are the top_k largest logits in
    descending order, equal logits to the lower expert, NaN last; the
    weights are their softmax probabilities, divided by their sum with
    `normalize` (sputnik/block/router.h). `weights_dtype`: None (the logits'
    dtype) or torch.float32, for weights and scores alike. One autograd
    function: top_experts carries no gradient, backward is one
    RouterTopKGrad over the gradients of the weights and of the scores."""
    weights_dtype = _router_args(logits, top_k, weights_dtype, "moe_router")
    return _Router.apply(logits, top_k, bool(normalize), weights_dtype,
                         bool(return_scores))


class _RouterAux(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, top_k, normalize, dtype):
        logits, top, weights = _router_forward(ctx, logits, top_k, normalize,
                                               dtype)
        tokens, e = logits.shape
        dev = logits.device
        score_sums = torch.empty(e, dtype=torch.float32, device=dev)
        z_sum = torch.empty(1, dtype=torch.float32, device=dev)
        groups = (tokens + ROUTER_AUX_TOKENS - 1) // ROUTER_AUX_TOKENS
        ws = _bt_workspace(groups * (e + 1) * 4, dev)
        RouterTopKAux(logits, top, weights, score_sums, ws, normalize, None,
                      z_sum)
        return weights, top, score_sums, z_sum

    @staticmethod
    def backward(ctx, dweights, _dtop, dscore_sums, dz_sum):
        args = _router_backward(ctx, dweights, dscore_sums, dz_sum)
        if args is None:
            return None, None, None, None
        logits, top, dweights, dlogits = args
        RouterTopKAuxGrad(logits, top, dweights, dlogits, ctx.normalize, None,
                          _contiguous(dscore_sums), _contiguous(dz_sum))
        return dlogits, None, None, None


def moe_router_aux(logits: torch.Tensor, top_k: int, normalize: bool = False,
                   weights_dtype=None):
    """moe_router with the statistics of the auxiliary losses: (expert_weights
    [tokens, top_k], top_experts int32 [tokens, top_k], score_sums fp32 [E],
    z_sum fp32 [1]). Weights and ids are moe_router's bit for bit; score_sums
    is the column sum over tokens of the softmax and z_sum the sum over
    tokens of logsumexp(logits)^2, both accumulated in fp32 from the
    unrounded values whatever the logits' dtype, without atomics (two calls
    on one input agree bit for bit). No [tokens, E] tensor is written. One
    autograd function that saves the logits and the ids: backward is one
    RouterTopKAuxGrad, which takes the gradients of score_sums and z_sum as
    an [E] vector and a device scalar (an absent one is not materialised).
    Feed them to load_balancing_loss and router_z_loss."""
    weights_dtype = _router_args(logits, top_k, weights_dtype,
                                 "moe_router_aux")
    return _RouterAux.apply(logits, top_k, bool(normalize), weights_dtype)


class _ScoreRouter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, bias, top_k, num_groups, topk_groups, normalize,
                scale, dtype, return_scores):
        logits, top, weights = _router_forward(ctx, logits, top_k, normalize,
                                               dtype)
        ctx.scale = scale
        scores = (torch.empty(logits.shape, dtype=dtype, device=logits.device)
                  if return_scores else None)
        RouterScoreTopK(logits, top, weights, bias, num_groups, topk_groups,
                        normalize, scale, scores)
        return (weights, top, scores) if return_scores else (weights, top)

    @staticmethod
    def backward(ctx, dweights, _dtop, dscores=None):
        args = _router_backward(ctx, dweights, dscores)
        if args is None:
            return (None,) * 9
        logits, top, dweights, dlogits = args
        RouterScoreTopKGrad(logits, top, dweights, dlogits, ctx.normalize,
                            ctx.scale, _contiguous(dscores))
        return (dlogits,) + (None,) * 8


def _score_args(logits, top_k, bias, num_groups, topk_groups, scale,
                what: str):
    """moe_score_router's checks beyond _router_args': the bias (detached,
    contiguous), the groups and the scale."""
    e = int(logits.shape[1])
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32:
            raise TypeError(f"{what}: bias must be an fp32 tensor")
        if tuple(bias.shape) != (e,):
            raise ValueError(f"{what}: bias is [num_experts]")
        bias = bias.detach().contiguous()
    for name, v in (("num_groups", num_groups), ("topk_groups", topk_groups)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{what}: {name} must be an int, not {v!r}")
    if (not 1 <= topk_groups <= num_groups <= ROUTER_MAX_GROUPS
            or e % num_groups != 0):
        raise ValueError(f"{what}: needs 1 <= topk_groups <= num_groups <= "
                         f"{ROUTER_MAX_GROUPS} and num_groups dividing {e} "
                         f"experts, not topk_groups = {topk_groups}, "
                         f"num_groups = {num_groups}")
    if top_k > topk_groups * (e // num_groups):
        raise ValueError(f"{what}: top_k = {top_k}, but {topk_groups} groups "
                         f"of {e // num_groups} experts are eligible")
    if (isinstance(scale, bool) or not isinstance(scale, (int, float))
            or not math.isfinite(scale)):
        raise ValueError(f"{what}: scale must be a finite number, not "
                         f"{scale!r}")
    return bias, float(scale)


def moe_score_router(logits: torch.Tensor, top_k: int,
                     bias: Optional[torch.Tensor] = None, num_groups: int = 1,
                     topk_groups: int = 1, normalize: bool = False,
                     scale: float = 1.0, weights_dtype=None,
                     return_scores: bool = False):
    """The choice of a router with sigmoid scores, a selection bias and a
    group limit (DeepSeek-V3's gate) from its logits [tokens, E]: the same
    returns as moe_router, (expert_weights [tokens, top_k], top_experts int32
    [tokens, top_k]) and, with `return_scores`, scores [tokens, E] (the
    sigmoid). The picks are the top_k largest sigmoid(logits) + bias (`bias`
    fp32 [E], None: 0) among the experts of the `topk_groups` best of
    `num_groups` groups, a group scoring the sum of its two largest; equal
    values to the lower expert, NaN last. The weights are the picks' scores
    without the bias, divided by their sum with `normalize`, times `scale`
    (sputnik/block/router.h, RouterScoreTopK). One autograd function,
    differentiable in the logits through weights and scores; the bias takes
    no gradient (router_bias_update moves it)."""
    what = "moe_score_router"
    weights_dtype = _router_args(logits, top_k, weights_dtype, what)
    bias, scale = _score_args(logits, top_k, bias, num_groups, topk_groups,
                              scale, what)
    return _ScoreRouter.apply(logits, bias, top_k, num_groups, topk_groups,
                              bool(normalize), scale, weights_dtype,
                              bool(return_scores))


def router_bias_update(bias: torch.Tensor, tokens_per_expert: torch.Tensor,
                       rate: float) -> torch.Tensor:
    """The auxiliary-loss-free balancing step on moe_score_router's bias, in
    place: bias += rate * sign(mean(tokens_per_expert) - tokens_per_expert),
    so an overloaded expert's bias falls and an underloaded one's rises.
    `tokens_per_expert` [E] (any integer or float dtype) is a route's
    (MoeRoute.tokens_per_expert). Plain torch on E elements, no host sync;
    returns `bias`."""
    if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32:
        raise TypeError("router_bias_update: bias must be an fp32 tensor")
    if not isinstance(tokens_per_expert, torch.Tensor):
        raise TypeError("router_bias_update: tokens_per_expert must be a "
                        "tensor")
    if bias.dim() != 1 or tokens_per_expert.shape != bias.shape:
        raise ValueError("router_bias_update: bias and tokens_per_expert are "
                         "[num_experts]")
    with torch.no_grad():
        load = tokens_per_expert.detach().to(torch.float32)
        bias.add_(torch.sign(load.mean() - load), alpha=float(rate))
    return bias


def _loss_sizes(tokens, top_k, what: str):
    for name, v in (("tokens", tokens), ("top_k", top_k)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"{what}: {name} must be an int >= 1, not {v!r}")


def load_balancing_loss(score_sums: torch.Tensor,
                        tokens_per_expert: torch.Tensor, tokens: int,
                        top_k: int, weight: float = 1.0) -> torch.Tensor:
    """weight * E / (tokens^2 * top_k) * sum_e tokens_per_expert_e *
    score_sums_e: MegaBlocks' batched_load_balancing_loss for one layer, from
    moe_router_aux's score_sums (fp32 [E]) and the route's tokens_per_expert
    ([E], any integer or float dtype; it carries no gradient). `weight` under
    perfect balance. Plain torch on E elements, no host sync; a 0-d fp32
    tensor."""
    if (not isinstance(score_sums, torch.Tensor)
            or score_sums.dtype != torch.float32):
        raise TypeError("load_balancing_loss: score_sums must be an fp32 "
                        "tensor")
    if not isinstance(tokens_per_expert, torch.Tensor):
        raise TypeError("load_balancing_loss: tokens_per_expert must be a "
                        "tensor")
    if score_sums.dim() != 1 or tokens_per_expert.shape != score_sums.shape:
        raise ValueError("load_balancing_loss: score_sums and "
                         "tokens_per_expert are [num_experts]")
    _loss_sizes(tokens, top_k, "load_balancing_loss")
    e = int(score_sums.numel())
    scale = float(weight) * e / (float(tokens) * float(tokens) * top_k)
    return scale * torch.dot(tokens_per_expert.detach().to(torch.float32),
                             score_sums)


def router_z_loss(z_sum: torch.Tensor, tokens: int,
                  weight: float = 1.0) -> torch.Tensor:
    """weight * z_sum / tokens: the router z-loss (the mean over tokens of
    logsumexp(logits)^2) from moe_router_aux's z_sum (fp32 [1]). A 0-d fp32
    tensor, no host sync."""
    if (not isinstance(z_sum, torch.Tensor) or z_sum.dtype != torch.float32):
        raise TypeError("router_z_loss: z_sum must be an fp32 tensor")
    if z_sum.numel() != 1:
        raise ValueError("router_z_loss: z_sum holds one element")
    _loss_sizes(tokens, 1, "router_z_loss")
    return (float(weight) / float(tokens)) * z_sum.reshape(())


@dataclass
class MoeAux:
    """What moe_layer_aux returns beside its output, the
    arguments of load_balancing_loss and router_z_loss: `score_sums` fp32 [E]
    and `z_sum` fp32 [1] (differentiable), `tokens_per_expert` int32 [E],
    and the layer's `tokens` and `top_k`."""

    score_sums: torch.Tensor
    z_sum: torch.Tensor
    tokens_per_expert: torch.Tensor
    tokens: int
    top_k: int


def _moe_layer(x, router_weight, w1, w2, top_k, activation, v1, rows,
               normalize, router_dtype, device_sort, returns: str, what: str,
               score=None, biases=(None, None, None)):
    """moe_layer's checks and chain. `returns`: "y", "scores" (moe_layer's
    return_scores) or "aux" (moe_layer_aux: routing through
    moe_router_aux). `score`: None, or moe_score_layer's (router_bias,
    num_groups, topk_groups, routed_scale): routing through
    moe_score_router."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError(f"{what}: x must be a 2-D tensor")
    _check_dtypes(x)
    if router_dtype is None:
        router_dtype = x.dtype
    elif router_dtype not in (x.dtype, torch.float32):
        raise TypeError(f"{what}: router_dtype must be {x.dtype} or "
                        "torch.float32")
    if (not isinstance(router_weight, torch.Tensor)
            or router_weight.dtype not in (x.dtype, torch.float32)):
        raise TypeError(f"{what}: router_weight must be {x.dtype} or "
                        "torch.float32")
    if router_weight.dim() != 2 or router_weight.shape[1] != x.shape[1]:
        raise ValueError(f"{what}: router_weight is [num_experts, d_model]")
    num_experts = int(router_weight.shape[0])
    if (isinstance(top_k, bool) or not isinstance(top_k, int)
            or not 1 <= top_k <= min(num_experts, ROUTER_MAX_TOP_K)):
        raise ValueError(f"{what}: top_k must be an int in [1, min("
                         f"{num_experts}, {ROUTER_MAX_TOP_K})], not {top_k!r}")
    if any(b is not None for b in biases):
        _check_moe_biases(x, w1, v1, num_experts, biases, what)
    logits = x.to(router_dtype) @ router_weight.to(router_dtype).t()
    if score is not None:
        bias, num_groups, topk_groups, scale = score
        out = moe_score_router(logits, top_k, bias, num_groups, topk_groups,
                               normalize, scale, None, returns == "scores")
    elif returns == "aux":
        out = moe_router_aux(logits, top_k, normalize, None)
    else:
        out = moe_router(logits, top_k, normalize, None, returns == "scores")
    top = out[1]
    if device_sort:
        top = moe_device_route(top, num_experts, rows)
    y, route = _moe_mlp(x, top, out[0], w1, w2, num_experts, activation, v1,
                        rows, *biases)
    if returns == "aux":
        return y, MoeAux(out[2], out[3], route.tokens_per_expert,
                         int(x.shape[0]), top_k)
    if returns == "scores":
        return y, out[2], route.tokens_per_expert
    return y


def moe_layer(x: torch.Tensor, router_weight: torch.Tensor, w1: torch.Tensor,
              w2: torch.Tensor, top_k: int, activation=None,
              v1: Optional[torch.Tensor] = None, rows: Optional[int] = None,
              normalize: bool = False, router_dtype=None,
              device_sort: bool = True, return_scores: bool = False):
    """A dropless MoE layer from activations to output: logits = x @
    router_weight.t() (torch; router_weight [E, d_model], the weight of an
    nn.Linear(d_model, E, bias=False)), moe_router(logits, top_k, normalize),
    then moe_mlp with its choice, routed by moe_device_route (`device_sort`
    False: by moe_route's torch.sort). `router_dtype` None: the logits in x's
    dtype; torch.float32: x and router_weight are converted and the logits,
    the softmax and the expert weights are fp32. With explicit `rows` the
    whole layer makes no host sync. Differentiable in x, router_weight, w1,
    v1 and w2. `return_scores`: returns (y, scores [tokens, E],
    tokens_per_expert int32 [E]), what MegaBlocks' load-balancing loss is
    formed from (moe_layer_aux returns the loss statistics instead, without
    the scores)."""
    return _moe_layer(x, router_weight, w1, w2, top_k, activation, v1, rows,
                      normalize, router_dtype, device_sort,
                      "scores" if return_scores else "y", "moe_layer")


def moe_layer_bias(x: torch.Tensor, router_weight: torch.Tensor,
                   w1: torch.Tensor, w2: torch.Tensor, top_k: int,
                   activation=None, v1: Optional[torch.Tensor] = None,
                   rows: Optional[int] = None, normalize: bool = False,
                   router_dtype=None, device_sort: bool = True,
                   return_scores: bool = False, *,
                   b1: Optional[torch.Tensor] = None,
                   bv1: Optional[torch.Tensor] = None,
                   b2: Optional[torch.Tensor] = None):
    """moe_layer with the expert biases of moe_mlp_bias (`b1`, `bv1`, `b2`):
    the same layer and the same leading arguments; with explicit `rows` it
    still makes no host sync. Without biases it is moe_layer, bit for bit."""
    return _moe_layer(x, router_weight, w1, w2, top_k, activation, v1, rows,
                      normalize, router_dtype, device_sort,
                      "scores" if return_scores else "y", "moe_layer_bias",
                      biases=(b1, bv1, b2))


def moe_layer_aux(x: torch.Tensor, router_weight: torch.Tensor,
                  w1: torch.Tensor, w2: torch.Tensor, top_k: int,
                  activation=None, v1: Optional[torch.Tensor] = None,
                  rows: Optional[int] = None, normalize: bool = False,
                  router_dtype=None, device_sort: bool = True):
    """moe_layer for training with the auxiliary losses: the same layer, the
    same arguments and the same output bit for bit, routed through
    moe_router_aux; returns (y, MoeAux), the arguments of
    load_balancing_loss and router_z_loss in fp32, without any [tokens, E]
    tensor beside the logits. With explicit `rows` the layer, both losses
    and the backward make no host sync."""
    return _moe_layer(x, router_weight, w1, w2, top_k, activation, v1, rows,
                      normalize, router_dtype, device_sort, "aux",
                      "moe_layer_aux")


def moe_layer_aux_bias(x: torch.Tensor, router_weight: torch.Tensor,
                       w1: torch.Tensor, w2: torch.Tensor, top_k: int,
                       activation=None, v1: Optional[torch.Tensor] = None,
                       rows: Optional[int] = None, normalize: bool = False,
                       router_dtype=None, device_sort: bool = True, *,
                       b1: Optional[torch.Tensor] = None,
                       bv1: Optional[torch.Tensor] = None,
                       b2: Optional[torch.Tensor] = None):
    """moe_layer_aux with the expert biases of moe_mlp_bias."""
    return _moe_layer(x, router_weight, w1, w2, top_k, activation, v1, rows,
                      normalize, router_dtype, device_sort, "aux",
                      "moe_layer_aux_bias", biases=(b1, bv1, b2))


def moe_score_layer(x: torch.Tensor, router_weight: torch.Tensor,
                    w1: torch.Tensor, w2: torch.Tensor, top_k: int,
                    activation=None, v1: Optional[torch.Tensor] = None,
                    rows: Optional[int] = None, normalize: bool = False,
                    router_dtype=None, device_sort: bool = True,
                    return_scores: bool = False,
                    router_bias: Optional[torch.Tensor] = None,
                    num_groups: int = 1, topk_groups: int = 1,
                    routed_scale: float = 1.0):
    """moe_layer with a sigmoid-score router: the same layer and the same
    leading arguments, routed through moe_score_router(logits, top_k,
    router_bias, num_groups, topk_groups, normalize, routed_scale) instead of
    moe_router. `return_scores` returns the sigmoid scores. With explicit
    `rows` the layer makes no host sync. `router_bias` takes no gradient:
    feed the route's tokens_per_expert (returned with `return_scores`) to
    router_bias_update."""
    return _moe_layer(x, router_weight, w1, w2, top_k, activation, v1, rows,
                      normalize, router_dtype, device_sort,
                      "scores" if return_scores else "y", "moe_score_layer",
                      (router_bias, num_groups, topk_groups, routed_scale))


def moe_score_layer_bias(x: torch.Tensor, router_weight: torch.Tensor,
                         w1: torch.Tensor, w2: torch.Tensor, top_k: int,
                         activation=None, v1: Optional[torch.Tensor] = None,
                         rows: Optional[int] = None, normalize: bool = False,
                         router_dtype=None, device_sort: bool = True,
                         return_scores: bool = False,
                         router_bias: Optional[torch.Tensor] = None,
                         num_groups: int = 1, topk_groups: int = 1,
                         routed_scale: float = 1.0, *,
                         b1: Optional[torch.Tensor] = None,
                         bv1: Optional[torch.Tensor] = None,
                         b2: Optional[torch.Tensor] = None):
    """moe_score_layer with the expert biases of moe_mlp_bias (the router's
    selection bias stays `router_bias`)."""
    return _moe_layer(x, router_weight, w1, w2, top_k, activation, v1, rows,
                      normalize, router_dtype, device_sort,
                      "scores" if return_scores else "y",
                      "moe_score_layer_bias",
                      (router_bias, num_groups, topk_groups, routed_scale),
                      biases=(b1, bv1, b2))


__all__ = ["MoeAux", "MoeRoute", "SparseMatrix", "dds", "dds_acc", "dsd", "dsd_acc",
           "expert_topology", "from_dense_mask", "glu_mlp", "mlp",
           "moe_device_route", "moe_layer", "moe_layer_aux", "moe_mlp",
           "moe_route",
           "moe_router", "moe_router_aux", "load_balancing_loss",
           "moe_score_router", "moe_score_layer", "router_bias_update",
           "router_z_loss",
           "moe_rows_bound", "padded_gather", "column_sum", "sdd_bias",
           "sdd_act_bias", "sdd_gated_bias", "mlp_bias", "glu_mlp_bias",
           "padded_scatter_bias", "moe_mlp_bias", "moe_layer_bias",
           "moe_layer_aux_bias", "moe_score_layer_bias",
           "padded_scatter", "sdd", "sdd_act", "sdd_gated",
           "Fp8Weight", "Fp8SparseMatrix", "quantize_rows", "quantize_sparse",
           "quantize_weight", "sdd_fp8", "dsd_fp8", "moe_mlp_fp8",
           "quantize_tiles", "quantize_sparse_t", "dsd_fp8_wgrad", "mlp_fp8",
           "moe_mlp_fp8_train",
           "topology_from_mask"]
