"""sputnik_amd — MI355X-native block-sparse matmul (DSD / DDS / SDD, block 128).

Python mirror of the reference's ``sputnik::block`` API (sputnik/sputnik.h,
sputnik/block/arguments.h) over the C-ABI of ``libsputnik.so``
(include/sputnik_amd.h). Names, argument meaning and the overload set follow
the reference:

    Matmul(BlockMatrix a, ta, Matrix b, tb, Matrix c)        DSD  dsd.h:10-15
    Matmul(Matrix a, ta, BlockMatrix b, tb, Matrix c)        DDS  dds.h:10-15
    Matmul(Matrix a, ta, Matrix b, tb, BlockMatrix c)        SDD  sdd.h:10-15
    MatmulEx(...)      (DSD/DDS, precomputed transposed metadata)
    RowIndices(a, row_indices), Transpose(a)
    AllocateTransposeBuffers(a), AllocateRowIndicesBuffer(a)

Device memory is held in torch tensors (plumbing only); every computation runs
in the HIP kernels of libsputnik.so. There is no CPU fallback: if the library
is missing, importing the compute entry points raises.
"""

from __future__ import annotations

import ctypes
import enum
import os
from dataclasses import dataclass, field
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SPUTNIK_AMD_LIB") or os.path.join(_HERE, "libsputnik.so")

hipSuccess = 0
hipErrorInvalidValue = 1
hipErrorNotSupported = 801


class SputnikError(RuntimeError):
    """A non-zero hipError_t returned by libsputnik."""

    def __init__(self, code: int, what: str):
        super().__init__(f"{what} failed with hipError_t {code}")
        self.code = code


class BlockSize(enum.IntEnum):
    """reference sputnik/block/arguments.h:13-19"""

    kNone = 0
    k16 = 16
    k32 = 32
    k64 = 64
    k128 = 128


def AsInt(b) -> int:  # noqa: N802 (reference name)
    b = int(b)
    return b if b in (16, 32, 64, 128) else 0


class _CBlockMatrix(ctypes.Structure):
    """sputnik_block_matrix_t — byte-identical to the C++ BlockMatrix (88 B)."""

    _fields_ = [
        ("rows", ctypes.c_int32),
        ("cols", ctypes.c_int32),
        ("nonzeros", ctypes.c_int32),
        ("block_size", ctypes.c_int32),
        ("data", ctypes.c_void_p),
        ("offsets", ctypes.c_void_p),
        ("indices", ctypes.c_void_p),
        ("offsets_t", ctypes.c_void_p),
        ("indices_t", ctypes.c_void_p),
        ("block_offsets", ctypes.c_void_p),
        ("row_indices", ctypes.c_void_p),
        ("bitmask", ctypes.c_void_p),
        ("create_metadata", ctypes.c_uint8),
    ]


class _CMatrix(ctypes.Structure):
    """sputnik_matrix_t (16 B)."""

    _fields_ = [
        ("rows", ctypes.c_int32),
        ("cols", ctypes.c_int32),
        ("data", ctypes.c_void_p),
    ]


_P = ctypes.c_void_p
_SIGNATURES = {
    "sputnik_dsd": [_P, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_int, _P],
    "sputnik_dsd_ex": [_P, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_int, _P],
    "sputnik_dds": [_P, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_int, _P],
    "sputnik_dds_ex": [_P, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_int, _P],
    "sputnik_sdd": [_P, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_int, _P],
    # accumulating DSD / DDS: (..., dtype, c_type, stream)
    "sputnik_dsd_acc": [_P, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_int,
                        ctypes.c_int, _P],
    "sputnik_dsd_ex_acc": [_P, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_int,
                           ctypes.c_int, _P],
    "sputnik_dds_acc": [_P, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_int,
                        ctypes.c_int, _P],
    "sputnik_dds_ex_acc": [_P, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_int,
                           ctypes.c_int, _P],
    # SDD activation products: (a, ta, b, tb, c, act, z, dtype, ws, ws_bytes,
    # stream); the elementwise stage alone: (z, h, n, act, dtype, stream) and
    # (g, z, out, n, act, dtype, stream)
    "sputnik_sdd_act": [_P, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_int,
                        _P, ctypes.c_int, _P, ctypes.c_size_t, _P],
    "sputnik_sdd_act_grad": [_P, ctypes.c_int, _P, ctypes.c_int, _P,
                             ctypes.c_int, _P, ctypes.c_int, _P,
                             ctypes.c_size_t, _P],
    "sputnik_block_activation": [_P, _P, ctypes.c_longlong, ctypes.c_int,
                                 ctypes.c_int, _P],
    "sputnik_block_activation_grad": [_P, _P, _P, ctypes.c_longlong,
                                      ctypes.c_int, ctypes.c_int, _P],
    "sputnik_sdd_act_route": [_P, ctypes.c_int, _P, ctypes.c_int, _P],
    # gated SDD products: (a, ta, b, tb, c, act, gate, up[, up_grad], dtype,
    # ws, ws_bytes, stream); the elementwise stages alone: (u, g, out, n, act,
    # dtype, stream) and (d, g, u, dg, du, n, act, dtype, stream)
    "sputnik_sdd_gated": [_P, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_int,
                          _P, _P, ctypes.c_int, _P, ctypes.c_size_t, _P],
    "sputnik_sdd_gated_grad": [_P, ctypes.c_int, _P, ctypes.c_int, _P,
                               ctypes.c_int, _P, _P, _P, ctypes.c_int, _P,
                               ctypes.c_size_t, _P],
    "sputnik_block_gate": [_P, _P, _P, ctypes.c_longlong, ctypes.c_int,
                           ctypes.c_int, _P],
    "sputnik_block_gate_grad": [_P, _P, _P, _P, _P, ctypes.c_longlong,
                                ctypes.c_int, ctypes.c_int, _P],
    # SDD with a column bias: (a, ta, b, tb, c, bias, [act, side buffers,]
    # dtype, ws, ws_bytes, stream); column sums: (s, dtype, out, stream)
    "sputnik_sdd_bias": [_P, ctypes.c_int, _P, ctypes.c_int, _P, _P,
                         ctypes.c_int, _P, ctypes.c_size_t, _P],
    "sputnik_sdd_bias_act": [_P, ctypes.c_int, _P, ctypes.c_int, _P, _P,
                             ctypes.c_int, _P, ctypes.c_int, _P,
                             ctypes.c_size_t, _P],
    "sputnik_sdd_bias_gated": [_P, ctypes.c_int, _P, ctypes.c_int, _P, _P,
                               ctypes.c_int, _P, _P, ctypes.c_int, _P,
                               ctypes.c_size_t, _P],
    "sputnik_block_column_sum": [_P, ctypes.c_int, _P, _P],
    "sputnik_ssd": [_P, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_int, _P],
    "sputnik_ssd_ex": [_P, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_int, _P],
    "sputnik_sds": [_P, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_int, _P],
    "sputnik_sds_ex": [_P, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_int, _P],
    "sputnik_dss": [_P, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_int, _P],
    "sputnik_dss_ex": [_P, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_int, _P],
    "sputnik_row_indices": [_P, _P, _P],
    "sputnik_transpose": [_P, _P],
    "sputnik_mask_to_bcsr": [_P, ctypes.c_int, ctypes.c_int, _P, _P, _P],
    "sputnik_expert_topology": [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                _P, _P, _P],
    # MoE token permutation: (bin_ids, n, experts, bins, tokens_per_expert,
    # padded_bins, stream); (indices, bin_ids, bins, padded_bins, n, experts,
    # rows, row_of, stream); (x, indices, bins, padded_bins, weights, out,
    # tokens, hidden, top_k, experts, rows, dtype, weights_dtype, stream);
    # (y, row_of, weights, out, tokens, hidden, top_k, rows, dtype,
    # weights_dtype, stream); (dout, y, row_of, dw, tokens, ..., stream)
    "sputnik_moe_bins": [_P, ctypes.c_int, ctypes.c_int, _P, _P, _P, _P],
    "sputnik_moe_row_map": [_P, _P, _P, _P, ctypes.c_int, ctypes.c_int,
                            ctypes.c_int, _P, _P],
    "sputnik_padded_gather": [_P, _P, _P, _P, _P, _P, ctypes.c_int,
                              ctypes.c_int, ctypes.c_int, ctypes.c_int,
                              ctypes.c_int, ctypes.c_int, ctypes.c_int, _P],
    "sputnik_padded_scatter": [_P, _P, _P, _P, ctypes.c_int, ctypes.c_int,
                               ctypes.c_int, ctypes.c_int, ctypes.c_int,
                               ctypes.c_int, _P],
    "sputnik_padded_scatter_wgrad": [_P, _P, _P, _P, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, _P],
    # the scatter with an output bias: (y, row_of, padded_bins, bias, weights,
    # out, tokens, hidden, top_k, experts, rows, dtype, weights_dtype,
    # stream); (dout, y, row_of, padded_bins, bias, dw, tokens, ..., stream);
    # (dout, indices, bins, weights, bias_grad, tokens, hidden, top_k,
    # experts, dtype, weights_dtype, stream)
    "sputnik_padded_scatter_bias": [_P, _P, _P, _P, _P, _P, ctypes.c_int,
                                    ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                    _P],
    "sputnik_padded_scatter_bias_wgrad": [_P, _P, _P, _P, _P, _P,
                                          ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, _P],
    "sputnik_padded_scatter_bias_grad": [_P, _P, _P, _P, _P, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, _P],
    # MoE router and device sort: (logits, top_experts, weights, scores,
    # tokens, experts, top_k, normalize, logits_dtype, weights_dtype, stream);
    # (logits, top_experts, dweights, dscores, dlogits, tokens, ..., stream);
    # (top_experts, n, experts, rows, indices, bin_ids, bins,
    # tokens_per_expert, padded_bins, row_of, workspace, bytes, stream)
    "sputnik_router_topk": [_P, _P, _P, _P, ctypes.c_int, ctypes.c_int,
                            ctypes.c_int, ctypes.c_int, ctypes.c_int,
                            ctypes.c_int, _P],
    "sputnik_router_topk_grad": [_P, _P, _P, _P, _P, ctypes.c_int,
                                 ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                 ctypes.c_int, ctypes.c_int, _P],
    # the router with the loss statistics: (logits, top_experts, weights,
    # scores, score_sums, z_sum, tokens, ..., weights_dtype, workspace, bytes,
    # stream); (logits, top_experts, dweights, dscores, dscore_sums, dz_sum,
    # dlogits, tokens, ..., stream)
    "sputnik_router_aux_workspace_bytes": [ctypes.c_int, ctypes.c_int],
    "sputnik_router_topk_aux": [_P, _P, _P, _P, _P, _P, ctypes.c_int,
                                ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                ctypes.c_int, ctypes.c_int, _P,
                                ctypes.c_size_t, _P],
    "sputnik_router_topk_aux_grad": [_P, _P, _P, _P, _P, _P, _P, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, _P],
    # the sigmoid-score router: (logits, bias, top_experts, weights, scores,
    # tokens, experts, top_k, num_groups, topk_groups, normalize, scale,
    # logits_dtype, weights_dtype, stream); (logits, top_experts, dweights,
    # dscores, dlogits, tokens, experts, top_k, normalize, scale, ..., stream)
    "sputnik_router_score_topk": [_P, _P, _P, _P, _P, ctypes.c_int,
                                  ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                  ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                  ctypes.c_int, ctypes.c_int, _P],
    "sputnik_router_score_topk_grad": [_P, _P, _P, _P, _P, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_float,
                                       ctypes.c_int, ctypes.c_int, _P],
    "sputnik_moe_sort_workspace_bytes": [ctypes.c_int, ctypes.c_int],
    "sputnik_moe_sort": [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P,
                         _P, _P, _P, _P, _P, ctypes.c_size_t, _P],
    # fp8 products: (x, rows, cols, [act,] q, scales, pow2, dtype, stream);
    # gated: (x, gate, rows, cols, act, q, ...); (w, k, n, transpose, q,
    # scales, pow2, dtype, stream); (aq, a_scales, k, bq, b_scales, c, dtype,
    # stream); (s, s_scales, bq, b_scales, c, dtype, stream)
    "sputnik_quantize_rows": [_P, ctypes.c_int, ctypes.c_int, _P, _P,
                              ctypes.c_int, ctypes.c_int, _P],
    "sputnik_quantize_rows_act": [_P, ctypes.c_int, ctypes.c_int,
                                  ctypes.c_int, _P, _P, ctypes.c_int,
                                  ctypes.c_int, _P],
    "sputnik_quantize_rows_gated": [_P, _P, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_int, _P, _P, ctypes.c_int,
                                    ctypes.c_int, _P],
    "sputnik_quantize_weight": [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                _P, _P, ctypes.c_int, ctypes.c_int, _P],
    "sputnik_sdd_fp8": [_P, _P, ctypes.c_int, _P, _P, _P, ctypes.c_int, _P],
    "sputnik_dsd_fp8": [_P, _P, _P, _P, _P, ctypes.c_int, _P],
    # ... with the accumulation mode in front of the stream, and P itself:
    # (aq, bq, m, n, k, accumulate, p, stream)
    "sputnik_sdd_fp8_acc": [_P, _P, ctypes.c_int, _P, _P, _P, ctypes.c_int,
                            ctypes.c_int, _P],
    "sputnik_dsd_fp8_acc": [_P, _P, _P, _P, _P, ctypes.c_int, ctypes.c_int,
                            _P],
    "sputnik_fp8_interval_sums": [_P, _P, ctypes.c_int, ctypes.c_int,
                                  ctypes.c_int, ctypes.c_int, _P, _P],
    # the gradients' pieces: (x, rows, cols, q, scales, qt, scales_t, pow2,
    # dtype, stream); (s, stage, act, z, q, scales, qt, scales_t, pow2, dtype,
    # stream); (q, scales, k, n, qt, scales_t, stream); (s, s_scales, bq,
    # b_scales, c, dtype, out, add, accumulate, stream)
    "sputnik_quantize_tiles": [_P, ctypes.c_int, ctypes.c_int, _P, _P, _P, _P,
                               ctypes.c_int, ctypes.c_int, _P],
    "sputnik_quantize_blocks": [_P, ctypes.c_int, ctypes.c_int, _P, _P, _P,
                                _P, _P, ctypes.c_int, ctypes.c_int, _P],
    "sputnik_fp8_transpose_weight": [_P, _P, ctypes.c_int, ctypes.c_int, _P,
                                     _P, _P],
    "sputnik_dsd_fp8_wgrad": [_P, _P, _P, _P, _P, ctypes.c_int, ctypes.c_int,
                              ctypes.c_int, ctypes.c_int, _P],
    "sputnik_can_implement": [ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_int, _P],
    "sputnik_abi_block_matrix_size": [],
    "sputnik_abi_block_matrix_offset": [ctypes.c_int],
    "sputnik_abi_matrix_size": [],
    "sputnik_version": [],
    "sputnik_build_hash": [],
    "sputnik_bitmask": [_P, _P],
    "sputnik_bitmask_bytes": [_P],
    "sputnik_sdd_plan": [_P, ctypes.c_int, _P, ctypes.c_int, _P],
    "sputnik_pair_errors": [],
    "sputnik_debug_pair_fault": [ctypes.c_int],
    "sputnik_capture_workspaces": [],
    "sputnik_select_dsd_kernel": [ctypes.c_int],
    "sputnik_tuning_get": [ctypes.c_char_p],
    "sputnik_tuning_set": [ctypes.c_char_p, ctypes.c_int],
    "sputnik_dsd_plan": [_P, ctypes.c_int, _P, ctypes.c_int, _P, _P],
    "sputnik_sdd_kernel": [_P, ctypes.c_int, _P, ctypes.c_int, _P],
    "sputnik_dds_plan": [_P, ctypes.c_int, _P, ctypes.c_int, _P, _P],
    # caller-owned transposed-B workspaces
    "sputnik_sdd_ws": [_P, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_int,
                       _P, ctypes.c_size_t, _P],
    "sputnik_dsd_ws": [_P, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_int,
                       _P, ctypes.c_size_t, _P],
    "sputnik_dsd_ex_ws": [_P, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_int,
                          _P, ctypes.c_size_t, _P],
    "sputnik_sdd_workspace_bytes": [_P, ctypes.c_int, _P, ctypes.c_int, _P],
    "sputnik_dsd_workspace_bytes": [_P, ctypes.c_int, _P, ctypes.c_int, _P],
    "sputnik_set_stream_workspace": [_P, _P, ctypes.c_size_t],
    "sputnik_retained_bytes": [],
    "sputnik_release_workspaces": [],
    "sputnik_incall_events": [],
    "sputnik_bt_launches": [],
}
_RESTYPES = {
    "sputnik_abi_block_matrix_size": ctypes.c_size_t,
    "sputnik_abi_block_matrix_offset": ctypes.c_size_t,
    "sputnik_abi_matrix_size": ctypes.c_size_t,
    "sputnik_version": ctypes.c_char_p,
    "sputnik_build_hash": ctypes.c_char_p,
    "sputnik_bitmask_bytes": ctypes.c_size_t,
    "sputnik_debug_pair_fault": None,
    "sputnik_sdd_workspace_bytes": ctypes.c_size_t,
    "sputnik_dsd_workspace_bytes": ctypes.c_size_t,
    "sputnik_moe_sort_workspace_bytes": ctypes.c_size_t,
    "sputnik_router_aux_workspace_bytes": ctypes.c_size_t,
    "sputnik_retained_bytes": ctypes.c_size_t,
    "sputnik_release_workspaces": ctypes.c_size_t,
    "sputnik_incall_events": ctypes.c_ulonglong,
    "sputnik_bt_launches": ctypes.c_ulonglong,
}

_lib: Optional[ctypes.CDLL] = None


def lib() -> ctypes.CDLL:
    """Load libsputnik.so (built by `make -C sputnik_amd`). Raises if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` or "
                "`make -C sputnik_amd`. There is no CPU fallback.")
        # PyTorch ships its own HIP runtime (same soname as ROCm's). Load it
        # first so the library binds to that one copy; loading libsputnik.so
        # first would pull in /opt/rocm's runtime next to torch's.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        handle = ctypes.CDLL(LIB_PATH)
        for name, args in _SIGNATURES.items():
            fn = getattr(handle, name)
            fn.argtypes = args
            fn.restype = _RESTYPES.get(name, ctypes.c_int)
        _lib = handle
    return _lib


def _ptr(t) -> Optional[int]:
    if t is None:
        return None
    return t.data_ptr()


@dataclass
class Matrix:
    """Dense row-major matrix (reference arguments.h:155-162)."""

    rows: int
    cols: int
    data: object  # torch.Tensor (fp16/bf16), rows*cols elements

    def _c(self) -> _CMatrix:
        return _CMatrix(self.rows, self.cols, _ptr(self.data))


@dataclass
class BlockMatrix:
    """BCSR matrix (reference arguments.h:48-153). rows/cols/nonzeros in
    elements; offsets int32 [rows/b+1]; indices int16 [#blocks]; data holds
    #blocks row-major b x b blocks back to back."""

    rows: int
    cols: int
    block_size: int
    nonzeros: int
    data: object
    offsets: object
    indices: object
    offsets_t: object = None
    indices_t: object = None
    block_offsets: object = None
    row_indices: object = None
    bitmask: object = None
    create_metadata: bool = True

    @property
    def num_blocks(self) -> int:
        b = AsInt(self.block_size)
        return self.nonzeros // (b * b) if b else 0

    def _c(self) -> _CBlockMatrix:
        return _CBlockMatrix(
            self.rows, self.cols, self.nonzeros, int(self.block_size),
            _ptr(self.data), _ptr(self.offsets), _ptr(self.indices),
            _ptr(self.offsets_t), _ptr(self.indices_t),
            _ptr(self.block_offsets), _ptr(self.row_indices),
            _ptr(self.bitmask), 1 if self.create_metadata else 0)


def _dtype_code(t) -> int:
    import torch

    if t.dtype == torch.float16:
        return 0
    if t.dtype == torch.bfloat16:
        return 1
    raise TypeError(f"unsupported element type {t.dtype} (fp16 or bf16)")


def _stream(stream) -> Optional[int]:
    if stream is not None:
        return int(stream)
    import torch

    return torch.cuda.current_stream().cuda_stream


def _check(code: int, what: str) -> None:
    if code != hipSuccess:
        raise SputnikError(code, what)


def _workspace(ws):
    """(pointer, bytes) of a caller-owned workspace tensor: any dtype, on
    the device, contiguous. Raises before any HIP call otherwise."""
    if not hasattr(ws, "data_ptr") or not hasattr(ws, "element_size"):
        raise TypeError("workspace must be a torch tensor")
    if not ws.is_cuda:
        raise ValueError("workspace must be device memory (a cuda tensor), "
                         f"not {ws.device}")
    if not ws.is_contiguous():
        raise ValueError("workspace must be contiguous")
    return ws.data_ptr(), ws.numel() * ws.element_size()


def _call(ex: bool, a, transpose_a: bool, b, transpose_b: bool, c, stream,
          workspace=None):
    ws = _workspace(workspace) if workspace is not None else None
    L = lib()
    ta, tb = int(bool(transpose_a)), int(bool(transpose_b))
    if isinstance(a, BlockMatrix) and isinstance(b, Matrix) and isinstance(c, Matrix):
        ca, cb, cc = a._c(), b._c(), c._c()
        if ws is not None:
            fn = L.sputnik_dsd_ex_ws if ex else L.sputnik_dsd_ws
            code = fn(ctypes.byref(ca), ta, ctypes.byref(cb), tb,
                      ctypes.byref(cc), _dtype_code(b.data), ws[0], ws[1],
                      _stream(stream))
            _check(code, "dsd")
            return
        fn = L.sputnik_dsd_ex if ex else L.sputnik_dsd
        code = fn(ctypes.byref(ca), ta, ctypes.byref(cb), tb, ctypes.byref(cc),
                  _dtype_code(b.data), _stream(stream))
        _check(code, "dsd")
        return
    if ws is not None and not (not ex and isinstance(a, Matrix)
                               and isinstance(b, Matrix)
                               and isinstance(c, BlockMatrix)):
        raise TypeError("workspace applies to SDD and DSD only")
    if isinstance(a, Matrix) and isinstance(b, BlockMatrix) and isinstance(c, Matrix):
        ca, cb, cc = a._c(), b._c(), c._c()
        fn = L.sputnik_dds_ex if ex else L.sputnik_dds
        code = fn(ctypes.byref(ca), ta, ctypes.byref(cb), tb, ctypes.byref(cc),
                  _dtype_code(a.data), _stream(stream))
        _check(code, "dds")
        return
    if (not ex and isinstance(a, Matrix) and isinstance(b, Matrix)
            and isinstance(c, BlockMatrix)):
        ca, cb, cc = a._c(), b._c(), c._c()
        if ws is not None:
            code = L.sputnik_sdd_ws(ctypes.byref(ca), ta, ctypes.byref(cb), tb,
                                    ctypes.byref(cc), _dtype_code(a.data),
                                    ws[0], ws[1], _stream(stream))
            _check(code, "sdd")
            return
        code = L.sputnik_sdd(ctypes.byref(ca), ta, ctypes.byref(cb), tb,
                             ctypes.byref(cc), _dtype_code(a.data),
                             _stream(stream))
        _check(code, "sdd")
        return
    if (isinstance(a, BlockMatrix) and isinstance(b, Matrix)
            and isinstance(c, BlockMatrix)):
        ca, cb, cc = a._c(), b._c(), c._c()
        fn = L.sputnik_ssd_ex if ex else L.sputnik_ssd
        code = fn(ctypes.byref(ca), ta, ctypes.byref(cb), tb, ctypes.byref(cc),
                  _dtype_code(b.data), _stream(stream))
        _check(code, "ssd")
        return
    if (isinstance(a, Matrix) and isinstance(b, BlockMatrix)
            and isinstance(c, BlockMatrix)):
        ca, cb, cc = a._c(), b._c(), c._c()
        fn = L.sputnik_sds_ex if ex else L.sputnik_sds
        code = fn(ctypes.byref(ca), ta, ctypes.byref(cb), tb, ctypes.byref(cc),
                  _dtype_code(a.data), _stream(stream))
        _check(code, "sds")
        return
    if (isinstance(a, BlockMatrix) and isinstance(b, BlockMatrix)
            and isinstance(c, Matrix)):
        ca, cb, cc = a._c(), b._c(), c._c()
        fn = L.sputnik_dss_ex if ex else L.sputnik_dss
        code = fn(ctypes.byref(ca), ta, ctypes.byref(cb), tb, ctypes.byref(cc),
                  _dtype_code(c.data), _stream(stream))
        _check(code, "dss")
        return
    raise TypeError("no Matmul overload for these operand kinds")


def Matmul(a, transpose_a, b, transpose_b, c, stream=None,  # noqa: N802
           workspace=None):
    """DSD / DDS / SDD / SSD / SDS / DSS by operand kinds, like the C++
    overload set. `workspace` (SDD and DSD): a device tensor of any dtype
    with at least sdd_workspace_bytes / dsd_workspace_bytes bytes for the
    transposed copy of B, so the call allocates and synchronises nothing
    (include/sputnik_amd.h, "Caller-owned workspaces"); it must outlive the
    work enqueued with it. None: the plain entry points."""
    _call(False, a, transpose_a, b, transpose_b, c, stream, workspace)


def MatmulEx(a, transpose_a, b, transpose_b, c, stream=None,  # noqa: N802
             workspace=None):
    """DSD / DDS / SSD / SDS / DSS with the transposed metadata already
    present. `workspace` (DSD) as in Matmul."""
    _call(True, a, transpose_a, b, transpose_b, c, stream, workspace)


SPUTNIK_OUT_OPERAND = 0
SPUTNIK_OUT_F32 = 1


def _acc_c_type(operand, c) -> int:
    """c_type of an accumulating call from c's tensor dtype: the operands'
    dtype or torch.float32. TypeError otherwise, before any library call."""
    import torch

    if not isinstance(c, Matrix):
        raise TypeError("MatmulAccumulate needs a dense c (there is no "
                        "accumulating SDD / SSD / SDS)")
    cd = getattr(c.data, "dtype", None)
    if cd == torch.float32:
        return SPUTNIK_OUT_F32
    if cd == operand.dtype:
        return SPUTNIK_OUT_OPERAND
    raise TypeError(f"c is {cd}: an accumulating product takes a c of the "
                    f"operands' dtype ({operand.dtype}) or torch.float32")


def _call_acc(ex: bool, a, transpose_a: bool, b, transpose_b: bool, c, stream):
    ta, tb = int(bool(transpose_a)), int(bool(transpose_b))
    if isinstance(c, BlockMatrix):
        raise TypeError("MatmulAccumulate needs a dense c (there is no "
                        "accumulating SDD / SSD / SDS)")
    if isinstance(a, BlockMatrix) and isinstance(b, Matrix):
        dtype = _dtype_code(b.data)
        c_type = _acc_c_type(b.data, c)
        L = lib()
        ca, cb, cc = a._c(), b._c(), c._c()
        fn = L.sputnik_dsd_ex_acc if ex else L.sputnik_dsd_acc
        _check(fn(ctypes.byref(ca), ta, ctypes.byref(cb), tb, ctypes.byref(cc),
                  dtype, c_type, _stream(stream)), "dsd (accumulate)")
        return
    if isinstance(a, Matrix) and isinstance(b, BlockMatrix):
        dtype = _dtype_code(a.data)
        c_type = _acc_c_type(a.data, c)
        L = lib()
        ca, cb, cc = a._c(), b._c(), c._c()
        fn = L.sputnik_dds_ex_acc if ex else L.sputnik_dds_acc
        _check(fn(ctypes.byref(ca), ta, ctypes.byref(cb), tb, ctypes.byref(cc),
                  dtype, c_type, _stream(stream)), "dds (accumulate)")
        return
    raise TypeError("no MatmulAccumulate overload for these operand kinds "
                    "(DSD and DDS only)")


def MatmulAccumulate(a, transpose_a, b, transpose_b, c, stream=None):  # noqa: N802
    """c += op(a) op(b) for DSD / DDS (by operand kinds, as Matmul), rounded
    once after the add. c.data is a tensor of the operands' dtype or of
    torch.float32 (rows x cols); anything else raises TypeError before the
    library is called, and so does a sparse c. Where the sparse operand has
    no blocks c is not touched; c must not overlap a or b. Always the 8-wave
    kernel: no 4-wave kernel, split mode or transposed-B workspace
    (sputnik/block/accumulate.h)."""
    _call_acc(False, a, transpose_a, b, transpose_b, c, stream)


def MatmulAccumulateEx(a, transpose_a, b, transpose_b, c, stream=None):  # noqa: N802
    """MatmulAccumulate with the transposed metadata already present."""
    _call_acc(True, a, transpose_a, b, transpose_b, c, stream)


SPUTNIK_ACT_RELU = 0
SPUTNIK_ACT_GELU = 1
SPUTNIK_ACT_SILU = 2
_ACT_NAMES = {"relu": SPUTNIK_ACT_RELU, "gelu": SPUTNIK_ACT_GELU,
              "silu": SPUTNIK_ACT_SILU}


def _act_code(activation) -> int:
    """SPUTNIK_ACT_* from a constant or a name ("relu", "gelu": the tanh
    form, "silu"). ValueError otherwise, before any library call."""
    if isinstance(activation, str):
        if activation in _ACT_NAMES:
            return _ACT_NAMES[activation]
    elif isinstance(activation, int) and not isinstance(activation, bool):
        if activation in _ACT_NAMES.values():
            return int(activation)
    raise ValueError(f"unknown activation {activation!r}: one of "
                     f"{sorted(_ACT_NAMES)} or SPUTNIK_ACT_RELU/GELU/SILU")


def _act_buffer(t, dtype, numel: int, what: str):
    """A block-data buffer of an activation call: `dtype`, `numel` elements,
    contiguous. Raises before any library call."""
    td = getattr(t, "dtype", None)
    if td != dtype:
        raise TypeError(f"{what} is {td}, expected {dtype}")
    if int(t.numel()) != numel:
        raise ValueError(f"{what} holds {int(t.numel())} elements, expected "
                         f"{numel}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")


def _sdd_act_operands(a, b, c, what: str) -> int:
    if not (isinstance(a, Matrix) and isinstance(b, Matrix)
            and isinstance(c, BlockMatrix)):
        raise TypeError(f"{what} is an SDD: dense a and b, sparse c")
    dtype = _dtype_code(a.data)
    for name, m in (("b", b), ("c", c)):
        md = getattr(m.data, "dtype", None)
        if md != a.data.dtype:
            raise TypeError(f"{what}: {name} is {md}, a is {a.data.dtype}")
    return dtype


# The SDD epilogue products: Python name -> (C entry point, error label).
_SDD_EPILOGUES = {
    "MatmulActivation": ("sputnik_sdd_act", "sdd (activation)"),
    "MatmulActivationGrad": ("sputnik_sdd_act_grad", "sdd (activation grad)"),
    "MatmulGated": ("sputnik_sdd_gated", "sdd (gated)"),
    "MatmulGatedGrad": ("sputnik_sdd_gated_grad", "sdd (gated grad)"),
}


def _call_sdd_epilogue(what: str, a, transpose_a, b, transpose_b, c,
                       activation, sides, stream, workspace):
    """One SDD epilogue product. `sides`: its side buffers in the C entry
    point's order, as (name, tensor, message); a tensor that is None raises
    TypeError(message) where there is a message, and is optional otherwise
    (buffers that share a message are required together, at the first)."""
    act = _act_code(activation)
    dtype = _sdd_act_operands(a, b, c, what)
    for i, (name, t, needs) in enumerate(sides):
        if needs and any(u is None for _, u, m in sides[i:] if m == needs):
            raise TypeError(needs)
        if t is not None:
            _act_buffer(t, a.data.dtype, int(c.nonzeros), name)
    ws = _workspace(workspace) if workspace is not None else (None, 0)
    fn, label = _SDD_EPILOGUES[what]
    ca, cb, cc = a._c(), b._c(), c._c()
    _check(getattr(lib(), fn)(
        ctypes.byref(ca), int(bool(transpose_a)), ctypes.byref(cb),
        int(bool(transpose_b)), ctypes.byref(cc), act,
        *(_ptr(t) for _, t, _ in sides), dtype, ws[0], ws[1],
        _stream(stream)), label)


def MatmulActivation(a, transpose_a, b, transpose_b, c, activation,  # noqa: N802
                     pre_activation=None, stream=None, workspace=None):
    """SDD with the activation fused: c.data = H = act(Z), Z = op(a) op(b)
    rounded to the operand type, at c's blocks. `pre_activation` (optional):
    a contiguous tensor of c.nonzeros elements of the operands' dtype that
    receives Z in c's storage order. `activation`: "relu", "gelu" (the tanh
    form), "silu" or a SPUTNIK_ACT_* constant. H equals act(Z) of the stored
    Z bit for bit, whichever kernel runs (sputnik/block/activation.h).
    `workspace` as in Matmul. Type and size errors are raised before the
    library is called."""
    _call_sdd_epilogue("MatmulActivation", a, transpose_a, b, transpose_b, c,
                       activation,
                       [("pre_activation", pre_activation, None)], stream,
                       workspace)


def MatmulActivationGrad(a, transpose_a, b, transpose_b, c, activation,  # noqa: N802
                         pre_activation, stream=None, workspace=None):
    """SDD gated by the activation's derivative: c.data = round(op(a) op(b))
    * act'(Z) at c's blocks, Z = `pre_activation` as MatmulActivation stored
    it (required; it must not be c.data)."""
    what = "MatmulActivationGrad"
    _call_sdd_epilogue(what, a, transpose_a, b, transpose_b, c, activation,
                       [("pre_activation", pre_activation,
                         f"{what} needs the pre-activation the forward call "
                         "stored")], stream, workspace)


def _block_epilogue(fn: str, label: str, activation, ref: str, ins: dict,
                    outs: dict, stream):
    """One elementwise stage: `ins` / `outs` are its named buffers in the C
    entry point's order. ins[ref] sets the dtype and the size every other
    buffer must have; an output that is None is allocated like the first
    input. Raises before any library call. Returns the outputs."""
    import torch

    act = _act_code(activation)
    r = ins[ref]
    dtype = _dtype_code(r)
    if not r.is_contiguous():
        raise ValueError(f"{ref} must be contiguous")
    n = int(r.numel())
    for name, t in ins.items():
        if name != ref:
            _act_buffer(t, r.dtype, n, name)
    res = []
    for name, t in outs.items():
        if t is None:
            t = torch.empty_like(next(iter(ins.values())))
        else:
            _act_buffer(t, r.dtype, n, name)
        res.append(t)
    if len(res) == 2 and res[0] is res[1]:
        raise ValueError(f"{' and '.join(outs)} must be two tensors")
    _check(getattr(lib(), fn)(*(_ptr(t) for t in (*ins.values(), *res)), n,
                              act, dtype, _stream(stream)), label)
    return res


def BlockActivation(z, activation, out=None, stream=None):  # noqa: N802
    """out = act(z) elementwise over block data (sputnik_block_activation):
    the second kernel of MatmulActivation's two-kernel route, bit-identical
    to its fused route. `out` defaults to a new tensor; it may be `z`."""
    return _block_epilogue("sputnik_block_activation", "block activation",
                           activation, "z", {"z": z}, {"out": out}, stream)[0]


def BlockActivationGrad(g, z, activation, out=None, stream=None):  # noqa: N802
    """out = g * act'(z) elementwise over block data
    (sputnik_block_activation_grad), rounded once. `out` defaults to a new
    tensor; it may be `g`."""
    return _block_epilogue("sputnik_block_activation_grad",
                           "block activation grad", activation, "z",
                           {"g": g, "z": z}, {"out": out}, stream)[0]


def MatmulGated(a, transpose_a, b, transpose_b, c, activation, gate,  # noqa: N802
                up=None, stream=None, workspace=None):
    """SDD with a gate fused: c.data = H = U * act(G), U = op(a) op(b)
    rounded to the operand type, at c's blocks; G = `gate` (required), a
    contiguous tensor of c.nonzeros elements of the operands' dtype in c's
    storage order. `up` (optional): a tensor of the same kind that receives
    U. `activation` as in MatmulActivation. H equals BlockGate of the stored
    (U, G) bit for bit, whichever kernel runs (sputnik/block/gated.h). gate
    and up must not be c.data, a, b or each other. Type and size errors are
    raised before the library is called."""
    what = "MatmulGated"
    _call_sdd_epilogue(what, a, transpose_a, b, transpose_b, c, activation,
                       [("gate", gate, f"{what} needs the gate"),
                        ("up", up, None)], stream, workspace)


def MatmulGatedGrad(a, transpose_a, b, transpose_b, c, activation, gate,  # noqa: N802
                    up, up_grad, stream=None, workspace=None):
    """The gradient pair of MatmulGated from one product: with D = op(a)
    op(b) rounded to the operand type, up_grad = D * act(G) and c.data =
    D * U * act'(G), G = `gate`, U = `up` as MatmulGated stored it (all three
    required). `up_grad` may be `up` itself (in place); no other two buffers
    may coincide."""
    what = "MatmulGatedGrad"
    both = f"{what} needs up, as MatmulGated stored it, and up_grad"
    _call_sdd_epilogue(what, a, transpose_a, b, transpose_b, c, activation,
                       [("gate", gate, f"{what} needs the gate"),
                        ("up", up, both), ("up_grad", up_grad, both)], stream,
                       workspace)


def BlockGate(u, g, activation, out=None, stream=None):  # noqa: N802
    """out = u * act(g) elementwise over block data (sputnik_block_gate),
    rounded once: the second kernel of MatmulGated's two-kernel route,
    bit-identical to its fused route. `out` defaults to a new tensor; it may
    be `u` or `g`."""
    return _block_epilogue("sputnik_block_gate", "block gate", activation,
                           "u", {"u": u, "g": g}, {"out": out}, stream)[0]


def BlockGateGrad(d, g, u, activation, dg=None, du=None, stream=None):  # noqa: N802
    """(dg, du) with dg = d * u * act'(g) and du = d * act(g) elementwise over
    block data (sputnik_block_gate_grad), each rounded once. `dg` and `du`
    default to new tensors; dg may be `d`, du may be `u` (in place); they
    must be two tensors."""
    dg, du = _block_epilogue("sputnik_block_gate_grad", "block gate grad",
                             activation, "d", {"d": d, "g": g, "u": u},
                             {"dg": dg, "du": du}, stream)
    return dg, du


def _column_bias(bias, c, dtype, what: str) -> None:
    """A column bias of an SDD: 1-D, c.cols elements of `dtype`, contiguous
    (any 2-byte alignment: a slice of a longer tensor will do). Raises before
    any library call."""
    if bias is None:
        raise TypeError(f"{what} needs a bias; without one call the "
                        "bias-free product")
    _act_buffer(bias, dtype, int(c.cols), "bias")
    if bias.dim() != 1:
        raise ValueError(f"bias has shape {tuple(bias.shape)}, expected "
                         f"[{int(c.cols)}]")


def _call_sdd_bias(fn: str, label: str, a, transpose_a, b, transpose_b, c,
                   bias, tail, stream, workspace):
    """One bias product; `tail`: the arguments between bias and dtype."""
    dtype = _sdd_act_operands(a, b, c, label)
    _column_bias(bias, c, a.data.dtype, label)
    ws = _workspace(workspace) if workspace is not None else (None, 0)
    ca, cb, cc = a._c(), b._c(), c._c()
    _check(getattr(lib(), fn)(
        ctypes.byref(ca), int(bool(transpose_a)), ctypes.byref(cb),
        int(bool(transpose_b)), ctypes.byref(cc), _ptr(bias), *tail, dtype,
        ws[0], ws[1], _stream(stream)), label)


def MatmulBias(a, transpose_a, b, transpose_b, c, bias, stream=None,  # noqa: N802
               workspace=None):
    """SDD with a column bias: c.data = round(Z + bias[col]) at c's blocks,
    Z = op(a) op(b) rounded to the operand type, `bias` a 1-D tensor of
    c.cols elements of the operands' dtype indexed by c's logical column, at
    any 2-byte alignment (sputnik/block/bias.h). The result is the plain
    product followed by the add, bit for bit, whichever kernel runs."""
    _call_sdd_bias("sputnik_sdd_bias", "sdd (bias)", a, transpose_a, b,
                   transpose_b, c, bias, (), stream, workspace)


def MatmulBiasActivation(a, transpose_a, b, transpose_b, c, bias,  # noqa: N802
                         activation, pre_activation=None, stream=None,
                         workspace=None):
    """MatmulActivation on the biased product: Z = round(op(a) op(b)) +
    bias[col], rounded, c.data = act(Z); `pre_activation` (optional) receives
    that biased Z, which is what MatmulActivationGrad reads."""
    act = _act_code(activation)
    if pre_activation is not None:
        _act_buffer(pre_activation, a.data.dtype, int(c.nonzeros),
                    "pre_activation")
    _call_sdd_bias("sputnik_sdd_bias_act", "sdd (bias, activation)", a,
                   transpose_a, b, transpose_b, c, bias,
                   (act, _ptr(pre_activation)), stream, workspace)


def MatmulBiasGated(a, transpose_a, b, transpose_b, c, bias, activation,  # noqa: N802
                    gate, up=None, stream=None, workspace=None):
    """MatmulGated on the biased product: U = round(op(a) op(b)) +
    bias[col], rounded, c.data = U * act(G); `up` (optional) receives that
    biased U, which is what MatmulGatedGrad reads. G = `gate` (required)
    would itself come from MatmulBias with the gate's bias."""
    act = _act_code(activation)
    if gate is None:
        raise TypeError("MatmulBiasGated needs the gate")
    for name, t in (("gate", gate), ("up", up)):
        if t is not None:
            _act_buffer(t, a.data.dtype, int(c.nonzeros), name)
    _call_sdd_bias("sputnik_sdd_bias_gated", "sdd (bias, gated)", a,
                   transpose_a, b, transpose_b, c, bias,
                   (act, _ptr(gate), _ptr(up)), stream, workspace)


def BlockColumnSum(s, out, stream=None):  # noqa: N802
    """out[c] = the fp32 sum of column c over s's stored blocks, `out` a
    contiguous fp32 tensor of s.cols elements: the bias gradient of a sparse
    matrix (sputnik_block_column_sum). No atomics: two runs give the same
    bits. s needs its transposed metadata (AllocateTransposeBuffers +
    Transpose); without it the library returns hipErrorInvalidValue."""
    import torch

    if not isinstance(s, BlockMatrix):
        raise TypeError("BlockColumnSum takes a BlockMatrix")
    dtype = _dtype_code(s.data)
    _act_buffer(out, torch.float32, int(s.cols), "out")
    cs = s._c()
    _check(lib().sputnik_block_column_sum(ctypes.byref(cs), dtype, _ptr(out),
                                          _stream(stream)), "BlockColumnSum")


def sdd_act_route(a, transpose_a, b, transpose_b, c) -> int:
    """Route MatmulActivation[Grad] would take for this problem now: 1 the
    fused epilogue of the 8-wave kernel, 2 plain SDD plus the elementwise
    kernel, -1 rejected (sputnik_sdd_act_route; knob "sdd_act_route")."""
    ca, cb, cc = a._c(), b._c(), c._c()
    return int(lib().sputnik_sdd_act_route(
        ctypes.byref(ca), int(bool(transpose_a)), ctypes.byref(cb),
        int(bool(transpose_b)), ctypes.byref(cc)))


def sdd_workspace_bytes(a, transpose_a, b, transpose_b, c) -> int:
    """Bytes of transposed-B workspace this SDD would use (0: none needed;
    sputnik_sdd_workspace_bytes). Host-only."""
    ca, cb, cc = a._c(), b._c(), c._c()
    return int(lib().sputnik_sdd_workspace_bytes(
        ctypes.byref(ca), int(bool(transpose_a)), ctypes.byref(cb),
        int(bool(transpose_b)), ctypes.byref(cc)))


def dsd_workspace_bytes(a, transpose_a, b, transpose_b, c) -> int:
    """Bytes of transposed-B workspace this DSD would use (0: none needed;
    sputnik_dsd_workspace_bytes). Host-only."""
    ca, cb, cc = a._c(), b._c(), c._c()
    return int(lib().sputnik_dsd_workspace_bytes(
        ctypes.byref(ca), int(bool(transpose_a)), ctypes.byref(cb),
        int(bool(transpose_b)), ctypes.byref(cc)))


def set_stream_workspace(stream, workspace) -> None:
    """Registers `workspace` (a device tensor; None unregisters) as the
    transposed-B workspace of `stream` (a torch stream, a raw handle, or
    None for torch's current stream) on the current device
    (sputnik_set_stream_workspace). The caller keeps the tensor alive while
    it is registered and until the work enqueued with it has finished."""
    handle = getattr(stream, "cuda_stream", stream)
    ptr, nbytes = (None, 0) if workspace is None else _workspace(workspace)
    if workspace is not None and nbytes == 0:
        # (an empty tensor has no pointer to hand over, and a null pointer
        # would unregister: the C entry point's answer for zero bytes)
        raise SputnikError(hipErrorInvalidValue, "set_stream_workspace")
    _check(lib().sputnik_set_stream_workspace(_stream(handle), ptr, nbytes),
           "set_stream_workspace")


def retained_bytes() -> int:
    """Device memory the library holds on the current device
    (sputnik_retained_bytes)."""
    return int(lib().sputnik_retained_bytes())


def release_workspaces() -> int:
    """Frees the library-owned transposed-B buffers of the current device
    after a device synchronize; bytes freed (sputnik_release_workspaces)."""
    return int(lib().sputnik_release_workspaces())


def incall_events() -> int:
    """Allocations, frees and synchronizes the library has executed inside
    product calls so far (sputnik_incall_events)."""
    return int(lib().sputnik_incall_events())


def bt_launches() -> int:
    """Transposes of B enqueued for products so far (sputnik_bt_launches)."""
    return int(lib().sputnik_bt_launches())


def RowIndices(a: BlockMatrix, row_indices, stream=None):  # noqa: N802
    """reference sputnik/block/row_indices/row_indices.h:10"""
    ca = a._c()
    _check(lib().sputnik_row_indices(ctypes.byref(ca), _ptr(row_indices),
                                     _stream(stream)), "RowIndices")


def Transpose(a: BlockMatrix, stream=None):  # noqa: N802
    """reference sputnik/block/transpose/transpose.h:10 (on the device)."""
    ca = a._c()
    _check(lib().sputnik_transpose(ctypes.byref(ca), _stream(stream)),
           "Transpose")


def MaskToBcsr(mask, offsets, indices, stream=None):  # noqa: N802
    """Device block mask (uint8 [R, C]) -> BCSR offsets (int32 [R+1]) and
    ascending int16 indices (capacity >= nonzeros), the reference's
    mask -> CSR scan (matrix_utils.cu:254-289), stream-ordered."""
    rows, cols = int(mask.shape[0]), int(mask.shape[1])
    _check(lib().sputnik_mask_to_bcsr(_ptr(mask), rows, cols, _ptr(offsets),
                                      _ptr(indices), _stream(stream)),
           "MaskToBcsr")


def ExpertTopology(padded_bins, block_rows, blocks_per_expert, offsets,  # noqa: N802
                   indices, stream=None):
    """MegaBlocks dMoE topology on the device from cumulative padded bins
    (int32 [experts]); see include/sputnik_amd.h."""
    _check(lib().sputnik_expert_topology(
        _ptr(padded_bins), int(padded_bins.numel()), int(block_rows),
        int(blocks_per_expert), _ptr(offsets), _ptr(indices),
        _stream(stream)), "ExpertTopology")


SPUTNIK_WEIGHTS_OPERAND = 0
SPUTNIK_WEIGHTS_F32 = 1


def _moe_meta(t, numel, what: str) -> None:
    """An int32 routing tensor of `numel` elements (None: any), contiguous.
    Raises before any library call."""
    import torch

    td = getattr(t, "dtype", None)
    if td != torch.int32:
        raise TypeError(f"{what} is {td}, expected torch.int32")
    if numel is not None and int(t.numel()) != numel:
        raise ValueError(f"{what} holds {int(t.numel())} elements, expected "
                         f"{numel}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")


def _moe_matrix(t, dtype, cols, what: str) -> None:
    """A [*, cols] row matrix of a permutation call: 2-D, `dtype` (None:
    fp16 or bf16), contiguous. Raises before any library call."""
    if dtype is None:
        _dtype_code(t)
    elif getattr(t, "dtype", None) != dtype:
        raise TypeError(f"{what} is {getattr(t, 'dtype', None)}, expected "
                        f"{dtype}")
    if t.dim() != 2 or (cols is not None and int(t.shape[1]) != cols):
        raise ValueError(f"{what} has shape {tuple(t.shape)}, expected "
                         f"[rows, {'hidden' if cols is None else cols}]")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")


def _moe_sizes(tokens: int, top_k, rows: int, what: str) -> int:
    """top_k as an int >= 1 and rows a multiple of 128, or ValueError."""
    if isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 1:
        raise ValueError(f"{what}: top_k must be an int >= 1, not {top_k!r}")
    if rows % 128:
        raise ValueError(f"{what}: {rows} padded rows, not a multiple of 128")
    return tokens * top_k


def _moe_weights(w, operand_dtype, n: int, what: str) -> int:
    """SPUTNIK_WEIGHTS_* of a per-assignment weight tensor ([tokens, top_k]
    or flat, n elements, the operand dtype or fp32, contiguous)."""
    import torch

    wd = getattr(w, "dtype", None)
    if wd == torch.float32:
        code = SPUTNIK_WEIGHTS_F32
    elif wd == operand_dtype:
        code = SPUTNIK_WEIGHTS_OPERAND
    else:
        raise TypeError(f"{what} is {wd}, expected {operand_dtype} or "
                        "torch.float32")
    if int(w.numel()) != n:
        raise ValueError(f"{what} holds {int(w.numel())} elements, expected "
                         f"tokens * top_k = {n}")
    if not w.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    return code


def MoeBins(bin_ids, num_experts, bins, tokens_per_expert, padded_bins,  # noqa: N802
            stream=None):
    """bins, tokens_per_expert and padded_bins (int32 [num_experts]) from the
    sorted bin_ids (int32 [n]) on the device (sputnik_moe_bins;
    sputnik/block/moe.h)."""
    e = int(num_experts)
    _moe_meta(bin_ids, None, "bin_ids")
    for name, t in (("bins", bins), ("tokens_per_expert", tokens_per_expert),
                    ("padded_bins", padded_bins)):
        _moe_meta(t, e, name)
    _check(lib().sputnik_moe_bins(
        _ptr(bin_ids), int(bin_ids.numel()), e, _ptr(bins),
        _ptr(tokens_per_expert), _ptr(padded_bins), _stream(stream)),
        "MoeBins")


def MoeRowMap(indices, bin_ids, bins, padded_bins, rows, row_of,  # noqa: N802
              stream=None):
    """row_of (int32 [n]): the padded row of every assignment, -1 where the
    routing tensors put it outside [0, rows) (sputnik_moe_row_map)."""
    n, e = int(indices.numel()), int(bins.numel())
    _moe_meta(indices, None, "indices")
    _moe_meta(bin_ids, n, "bin_ids")
    _moe_meta(bins, None, "bins")
    _moe_meta(padded_bins, e, "padded_bins")
    _moe_meta(row_of, n, "row_of")
    if int(rows) % 128:
        raise ValueError(f"MoeRowMap: {rows} padded rows, not a multiple of "
                         "128")
    _check(lib().sputnik_moe_row_map(
        _ptr(indices), _ptr(bin_ids), _ptr(bins), _ptr(padded_bins), n, e,
        int(rows), _ptr(row_of), _stream(stream)), "MoeRowMap")


def PaddedGather(x, indices, bins, padded_bins, out, top_k, weights=None,  # noqa: N802
                 stream=None):
    """out [rows, hidden] = the rows of x [tokens, hidden] in padded expert
    order: out[row(i)] = x[indices[i] // top_k], bit for bit, or times
    weights[indices[i]] (rounded once) with `weights` ([tokens, top_k] or
    flat, x's dtype or fp32). Every other row of `out` is written as +0:
    `out` needs no initialisation (sputnik_padded_gather). Type and shape
    errors are raised before the library is called."""
    _moe_matrix(x, None, None, "x")
    dtype = _dtype_code(x)
    tokens, hidden = int(x.shape[0]), int(x.shape[1])
    _moe_matrix(out, x.dtype, hidden, "out")
    rows = int(out.shape[0])
    n = _moe_sizes(tokens, top_k, rows, "PaddedGather")
    _moe_meta(indices, n, "indices")
    _moe_meta(bins, None, "bins")
    _moe_meta(padded_bins, int(bins.numel()), "padded_bins")
    wcode = (SPUTNIK_WEIGHTS_OPERAND if weights is None
             else _moe_weights(weights, x.dtype, n, "weights"))
    _check(lib().sputnik_padded_gather(
        _ptr(x), _ptr(indices), _ptr(bins), _ptr(padded_bins), _ptr(weights),
        _ptr(out), tokens, hidden, top_k, int(bins.numel()), rows, dtype,
        wcode, _stream(stream)), "PaddedGather")


def _expert_bias(bias, dtype, hidden: int, what: str) -> int:
    """The number of experts of an output bias [E, hidden] of `dtype`."""
    _moe_matrix(bias, dtype, hidden, what)
    return int(bias.shape[0])


def _padded_scatter(what: str, y, row_of, out, top_k, weights, stream,
                    expert_bias=None) -> None:
    """PaddedScatter, or with expert_bias = (padded_bins, bias)
    PaddedScatterBias: the checks of both, then each one's own C symbol."""
    _moe_matrix(y, None, None, "y")
    dtype = _dtype_code(y)
    rows, hidden = int(y.shape[0]), int(y.shape[1])
    _moe_matrix(out, y.dtype, hidden, "out")
    tokens = int(out.shape[0])
    n = _moe_sizes(tokens, top_k, rows, what)
    _moe_meta(row_of, n, "row_of")
    if expert_bias is not None:
        padded_bins, bias = expert_bias
        e = _expert_bias(bias, y.dtype, hidden, "bias")
        _moe_meta(padded_bins, e, "padded_bins")
    wcode = (SPUTNIK_WEIGHTS_OPERAND if weights is None
             else _moe_weights(weights, y.dtype, n, "weights"))
    if expert_bias is None:
        code = lib().sputnik_padded_scatter(
            _ptr(y), _ptr(row_of), _ptr(weights), _ptr(out), tokens, hidden,
            top_k, rows, dtype, wcode, _stream(stream))
    else:
        code = lib().sputnik_padded_scatter_bias(
            _ptr(y), _ptr(row_of), _ptr(padded_bins), _ptr(bias),
            _ptr(weights), _ptr(out), tokens, hidden, top_k, e, rows, dtype,
            wcode, _stream(stream))
    _check(code, what)


def _padded_scatter_wgrad(what: str, dout, y, row_of, dw, top_k, stream,
                          expert_bias=None) -> None:
    """PaddedScatterWeightGrad, or with expert_bias = (padded_bins, bias)
    PaddedScatterBiasWeightGrad, as _padded_scatter."""
    _moe_matrix(dout, None, None, "dout")
    dtype = _dtype_code(dout)
    tokens, hidden = int(dout.shape[0]), int(dout.shape[1])
    _moe_matrix(y, dout.dtype, hidden, "y")
    rows = int(y.shape[0])
    n = _moe_sizes(tokens, top_k, rows, what)
    _moe_meta(row_of, n, "row_of")
    if expert_bias is not None:
        padded_bins, bias = expert_bias
        e = _expert_bias(bias, dout.dtype, hidden, "bias")
        _moe_meta(padded_bins, e, "padded_bins")
    wcode = _moe_weights(dw, dout.dtype, n, "dw")
    if expert_bias is None:
        code = lib().sputnik_padded_scatter_wgrad(
            _ptr(dout), _ptr(y), _ptr(row_of), _ptr(dw), tokens, hidden,
            top_k, rows, dtype, wcode, _stream(stream))
    else:
        code = lib().sputnik_padded_scatter_bias_wgrad(
            _ptr(dout), _ptr(y), _ptr(row_of), _ptr(padded_bins), _ptr(bias),
            _ptr(dw), tokens, hidden, top_k, e, rows, dtype, wcode,
            _stream(stream))
    _check(code, what)


def PaddedScatter(y, row_of, out, top_k, weights=None, stream=None):  # noqa: N802
    """out [tokens, hidden] = for every token the sum over its top_k padded
    rows of y [rows, hidden], read through row_of (int32 [tokens * top_k])
    and multiplied by `weights` when given; fp32 sum in ascending k, rounded
    once, no atomics (sputnik_padded_scatter). Type and shape errors are
    raised before the library is called."""
    _padded_scatter("PaddedScatter", y, row_of, out, top_k, weights, stream)


def PaddedScatterWeightGrad(dout, y, row_of, dw, top_k, stream=None):  # noqa: N802
    """dw[a] = dot(dout[a // top_k], y[row_of[a]]) in fp32, stored in dw's
    dtype (the operands' or fp32): the gradient of PaddedScatter with respect
    to its weights (sputnik_padded_scatter_wgrad). Type and shape errors are
    raised before the library is called."""
    _padded_scatter_wgrad("PaddedScatterWeightGrad", dout, y, row_of, dw,
                          top_k, stream)


def PaddedScatterBias(y, row_of, padded_bins, bias, out, top_k,  # noqa: N802
                      weights=None, stream=None):
    """PaddedScatter with an output bias [E, hidden] of y's dtype: out[t] =
    sum_k w_k * (y[row_k] + bias[e_k]) in fp32 (one add, one multiply, one
    accumulate per k, ascending k), rounded once. The expert e_k is read off
    the row through padded_bins (int32 [E]); an assignment whose row is out
    of range contributes zero, bias included
    (sputnik_padded_scatter_bias)."""
    _padded_scatter("PaddedScatterBias", y, row_of, out, top_k, weights,
                    stream, (padded_bins, bias))


def PaddedScatterBiasWeightGrad(dout, y, row_of, padded_bins, bias, dw,  # noqa: N802
                                top_k, stream=None):
    """dw[a] = dot(dout[a // top_k], y[row_of[a]] + bias[e]) in fp32, stored
    in dw's dtype: the gradient of PaddedScatterBias with respect to its
    weights (sputnik_padded_scatter_bias_wgrad)."""
    _padded_scatter_wgrad("PaddedScatterBiasWeightGrad", dout, y, row_of, dw,
                          top_k, stream, (padded_bins, bias))


def PaddedScatterBiasGrad(dout, indices, bins, bias_grad, top_k,  # noqa: N802
                          weights=None, stream=None):
    """bias_grad [E, hidden] (fp32) = for every expert the sum over its
    sorted positions i of weights[indices[i]] * dout[indices[i] // top_k]:
    the gradient of PaddedScatterBias with respect to its bias, from the
    unrounded fp32 products. No atomics: two runs give the same bits; an
    expert without tokens gives +0 (sputnik_padded_scatter_bias_grad)."""
    import torch

    _moe_matrix(dout, None, None, "dout")
    dtype = _dtype_code(dout)
    tokens, hidden = int(dout.shape[0]), int(dout.shape[1])
    n = _moe_sizes(tokens, top_k, 0, "PaddedScatterBiasGrad")
    e = _expert_bias(bias_grad, torch.float32, hidden, "bias_grad")
    _moe_meta(indices, n, "indices")
    _moe_meta(bins, e, "bins")
    wcode = (SPUTNIK_WEIGHTS_OPERAND if weights is None
             else _moe_weights(weights, dout.dtype, n, "weights"))
    _check(lib().sputnik_padded_scatter_bias_grad(
        _ptr(dout), _ptr(indices), _ptr(bins), _ptr(weights),
        _ptr(bias_grad), tokens, hidden, top_k, e, dtype, wcode,
        _stream(stream)), "PaddedScatterBiasGrad")


SPUTNIK_ROUTER_F16 = 0
SPUTNIK_ROUTER_BF16 = 1
SPUTNIK_ROUTER_F32 = 2
ROUTER_MAX_EXPERTS = 1024
ROUTER_MAX_TOP_K = 32
MOE_SORT_CHUNK = 1024


def _router_logits(t, what: str):
    """(SPUTNIK_ROUTER_* code, tokens, experts) of a [tokens, E] matrix of
    fp16, bf16 or fp32, contiguous, 1 <= E <= 1024. Raises before any library
    call."""
    import torch

    code = {torch.float16: SPUTNIK_ROUTER_F16,
            torch.bfloat16: SPUTNIK_ROUTER_BF16,
            torch.float32: SPUTNIK_ROUTER_F32}.get(getattr(t, "dtype", None))
    if code is None:
        raise TypeError(f"{what} is {getattr(t, 'dtype', None)}, expected "
                        "torch.float16, torch.bfloat16 or torch.float32")
    if t.dim() != 2:
        raise ValueError(f"{what} has shape {tuple(t.shape)}, expected "
                         "[tokens, num_experts]")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    tokens, e = int(t.shape[0]), int(t.shape[1])
    if not 1 <= e <= ROUTER_MAX_EXPERTS:
        raise ValueError(f"{what}: {e} experts, outside [1, "
                         f"{ROUTER_MAX_EXPERTS}]")
    return code, tokens, e


def _router_picks(top_experts, tokens: int, e: int, what: str) -> int:
    """top_k of an int32 [tokens, top_k] tensor, 1 <= top_k <= min(E, 32)."""
    _moe_meta(top_experts, None, "top_experts")
    if top_experts.dim() != 2 or int(top_experts.shape[0]) != tokens:
        raise ValueError(f"{what}: top_experts has shape "
                         f"{tuple(top_experts.shape)}, expected [{tokens}, "
                         "top_k]")
    k = int(top_experts.shape[1])
    if not 1 <= k <= min(e, ROUTER_MAX_TOP_K):
        raise ValueError(f"{what}: top_k = {k}, outside [1, min({e}, "
                         f"{ROUTER_MAX_TOP_K})]")
    return k


def _router_values(t, logits, shape, code, what: str) -> int:
    """SPUTNIK_WEIGHTS_* of a weights / scores tensor of `shape`: the logits'
    dtype or fp32, the same choice (`code`, None: free) as its companions."""
    import torch

    td = getattr(t, "dtype", None)
    if td == logits.dtype and code in (None, SPUTNIK_WEIGHTS_OPERAND):
        got = SPUTNIK_WEIGHTS_OPERAND
    elif td == torch.float32 and code in (None, SPUTNIK_WEIGHTS_F32):
        got = SPUTNIK_WEIGHTS_F32
    else:
        want = (f"{logits.dtype} or torch.float32" if code is None else
                "the dtype of the other weights / scores tensor")
        raise TypeError(f"{what} is {td}, expected {want}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} has shape {tuple(t.shape)}, expected "
                         f"{tuple(shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    return got


def _router_head(logits, top_experts, weights, scores, what: str, d=""):
    """(code, tokens, E, top_k, weights code) of a call's logits, picks,
    weights [tokens, top_k] and optional scores [tokens, E]; with d = "d" the
    last two are a gradient call's dweights and dscores."""
    code, tokens, e = _router_logits(logits, "logits")
    k = _router_picks(top_experts, tokens, e, what)
    wcode = _router_values(weights, logits, (tokens, k), None, d + "weights")
    if scores is not None:
        _router_values(scores, logits, (tokens, e), wcode, d + "scores")
    return code, tokens, e, k, wcode


def _router_dlogits(dlogits, logits) -> None:
    _router_values(dlogits, logits, tuple(logits.shape),
                   SPUTNIK_WEIGHTS_OPERAND, "dlogits")


def _workspace_bytes(workspace, need: int, what: str, device=None) -> int:
    """Bytes of a caller's workspace tensor (None: 0), contiguous, on
    `device` when given and at least `need`."""
    have = 0
    if workspace is not None:
        if not workspace.is_contiguous():
            raise ValueError("workspace must be contiguous")
        if device is not None and workspace.device != device:
            raise ValueError(f"workspace is on {workspace.device}, the "
                             f"logits on {device}")
        have = int(workspace.numel()) * int(workspace.element_size())
    if have < need:
        raise ValueError(f"{what}: a workspace of {have} bytes, "
                         f"{need} needed")
    return have


def RouterTopK(logits, top_experts, weights, normalize=False, scores=None,  # noqa: N802
               stream=None):
    """The router's choice from logits [tokens, E] (fp16, bf16 or fp32):
    top_experts int32 [tokens, top_k] (the top_k largest logits, descending,
    ties to the lower index, NaN below -inf), weights [tokens, top_k] (the
    softmax probabilities of the picks, divided by their sum with
    `normalize`) and, when given, scores [tokens, E] (the softmax). weights
    and scores share one dtype, the logits' or fp32
    (sputnik_router_topk; sputnik/block/router.h). Type and shape errors are
    raised before the library is called."""
    code, tokens, e, k, wcode = _router_head(
        logits, top_experts, weights, scores, "RouterTopK")
    _check(lib().sputnik_router_topk(
        _ptr(logits), _ptr(top_experts), _ptr(weights), _ptr(scores), tokens,
        e, k, int(bool(normalize)), code, wcode, _stream(stream)),
        "RouterTopK")


def RouterTopKGrad(logits, top_experts, dweights, dlogits, normalize=False,  # noqa: N802
                   dscores=None, stream=None):
    """dlogits [tokens, E] (the logits' dtype): the gradient of RouterTopK's
    weights (and scores, with `dscores`) with respect to the logits, the
    softmax recomputed from `logits`. A top_experts entry outside [0, E)
    contributes nothing, a duplicated one twice (sputnik_router_topk_grad).
    Type and shape errors are raised before the library is called."""
    code, tokens, e, k, wcode = _router_head(
        logits, top_experts, dweights, dscores, "RouterTopKGrad", "d")
    _router_dlogits(dlogits, logits)
    _check(lib().sputnik_router_topk_grad(
        _ptr(logits), _ptr(top_experts), _ptr(dweights), _ptr(dscores),
        _ptr(dlogits), tokens, e, k, int(bool(normalize)), code, wcode,
        _stream(stream)), "RouterTopKGrad")


ROUTER_AUX_TOKENS = 64     # sputnik::block::kRouterAuxTokens


def _router_stat(t, logits, numel: int, what: str) -> None:
    """An fp32 statistic of the auxiliary losses or its gradient: `numel`
    elements, 1-D, contiguous, on the logits' device."""
    import torch

    td = getattr(t, "dtype", None)
    if td != torch.float32:
        raise TypeError(f"{what} is {td}, expected torch.float32")
    if tuple(t.shape) != (numel,):
        raise ValueError(f"{what} has shape {tuple(t.shape)}, expected "
                         f"({numel},)")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    if t.device != logits.device:
        raise ValueError(f"{what} is on {t.device}, the logits on "
                         f"{logits.device}")


def router_aux_workspace_bytes(tokens: int, num_experts: int) -> int:
    """Bytes of workspace RouterTopKAux needs: ceil(tokens / 64) *
    (num_experts + 1) * 4 (sputnik_router_aux_workspace_bytes)."""
    tokens, e = int(tokens), int(num_experts)
    if tokens < 0 or not 1 <= e <= ROUTER_MAX_EXPERTS:
        raise ValueError(f"router_aux_workspace_bytes: tokens = {tokens} "
                         f"must be >= 0 and num_experts = {e} in [1, "
                         f"{ROUTER_MAX_EXPERTS}]")
    return int(lib().sputnik_router_aux_workspace_bytes(tokens, e))


def RouterTopKAux(logits, top_experts, weights, score_sums, workspace,  # noqa: N802
                  normalize=False, scores=None, z_sum=None, stream=None):
    """RouterTopK (the same top_experts, weights and scores, bit for bit)
    plus the statistics of the auxiliary losses in fp32, from the unrounded
    probabilities: score_sums fp32 [E] = the column sums of the softmax and,
    when given, z_sum fp32 [1] = the sum over tokens of logsumexp(logits)^2.
    No atomics: the sums are a function of the logits alone. `workspace`: a
    contiguous tensor of at least router_aux_workspace_bytes(tokens, E)
    bytes (None when that is 0); it needs no initialisation
    (sputnik_router_topk_aux; sputnik/block/router.h). Type, shape and device
    errors are raised before the library is called."""
    code, tokens, e, k, wcode = _router_head(
        logits, top_experts, weights, scores, "RouterTopKAux")
    _router_stat(score_sums, logits, e, "score_sums")
    if z_sum is not None:
        _router_stat(z_sum, logits, 1, "z_sum")
    need = ((tokens + ROUTER_AUX_TOKENS - 1) // ROUTER_AUX_TOKENS
            * (e + 1) * 4)
    have = _workspace_bytes(workspace, need, "RouterTopKAux", logits.device)
    _check(lib().sputnik_router_topk_aux(
        _ptr(logits), _ptr(top_experts), _ptr(weights), _ptr(scores),
        _ptr(score_sums), _ptr(z_sum), tokens, e, k, int(bool(normalize)),
        code, wcode, _ptr(workspace), have, _stream(stream)),
        "RouterTopKAux")


def RouterTopKAuxGrad(logits, top_experts, dweights, dlogits,  # noqa: N802
                      normalize=False, dscores=None, dscore_sums=None,
                      dz_sum=None, stream=None):
    """RouterTopKGrad with the gradients of RouterTopKAux's statistics:
    dscore_sums fp32 [E] is added to every row of dp, and dz_sum fp32 [1]
    (read on the device) adds 2 dz_sum logsumexp(logits_t) p_tj. Either may
    be None; with both None the result is RouterTopKGrad's bit for bit
    (sputnik_router_topk_aux_grad). Type, shape and device errors are raised
    before the library is called."""
    code, tokens, e, k, wcode = _router_head(
        logits, top_experts, dweights, dscores, "RouterTopKAuxGrad", "d")
    if dscore_sums is not None:
        _router_stat(dscore_sums, logits, e, "dscore_sums")
    if dz_sum is not None:
        _router_stat(dz_sum, logits, 1, "dz_sum")
    _router_dlogits(dlogits, logits)
    _check(lib().sputnik_router_topk_aux_grad(
        _ptr(logits), _ptr(top_experts), _ptr(dweights), _ptr(dscores),
        _ptr(dscore_sums), _ptr(dz_sum), _ptr(dlogits), tokens, e, k,
        int(bool(normalize)), code, wcode, _stream(stream)),
        "RouterTopKAuxGrad")


ROUTER_MAX_GROUPS = 64     # sputnik::block::kRouterMaxGroups


def _router_scale(scale, what: str) -> float:
    import math

    if (isinstance(scale, bool) or not isinstance(scale, (int, float))
            or not math.isfinite(scale)
            or not math.isfinite(ctypes.c_float(scale).value)):
        raise ValueError(f"{what}: scale must be a finite number (in fp32), "
                         f"not {scale!r}")
    return float(scale)


def _router_groups(e: int, k: int, num_groups, topk_groups, what: str) -> None:
    """RouterScoreTopK's limits on the groups: 1 <= topk_groups <= num_groups
    <= 64, E % num_groups == 0, top_k <= topk_groups * E / num_groups."""
    for name, v in (("num_groups", num_groups), ("topk_groups", topk_groups)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{what}: {name} must be an int, not {v!r}")
    if not 1 <= topk_groups <= num_groups <= ROUTER_MAX_GROUPS:
        raise ValueError(f"{what}: 1 <= topk_groups <= num_groups <= "
                         f"{ROUTER_MAX_GROUPS} does not hold for topk_groups "
                         f"= {topk_groups}, num_groups = {num_groups}")
    if e % num_groups != 0:
        raise ValueError(f"{what}: {e} experts do not divide into "
                         f"{num_groups} groups")
    if k > topk_groups * (e // num_groups):
        raise ValueError(f"{what}: top_k = {k}, but {topk_groups} groups of "
                         f"{e // num_groups} experts are eligible")


def _router_distinct(outs, ins, what: str) -> None:
    """No output (name, tensor) shares its address with an input or another
    output; absent and empty tensors are left out."""
    seen = {t.data_ptr(): name for name, t in ins
            if t is not None and int(t.numel()) > 0}
    for name, t in outs:
        if t is None or int(t.numel()) == 0:
            continue
        if t.data_ptr() in seen:
            raise ValueError(f"{what}: {name} aliases {seen[t.data_ptr()]}")
        seen[t.data_ptr()] = name


def RouterScoreTopK(logits, top_experts, weights, bias=None, num_groups=1,  # noqa: N802
                    topk_groups=1, normalize=False, scale=1.0, scores=None,
                    stream=None):
    """The choice of a router with sigmoid scores (DeepSeek-V3's) from logits
    [tokens, E] (fp16, bf16 or fp32): s = sigmoid(logits); top_experts int32
    [tokens, top_k] = the top_k largest s + bias (bias fp32 [E], None: 0)
    among the experts of the `topk_groups` best of `num_groups` groups of
    E / num_groups consecutive experts, a group's score being the sum of its
    two largest s + bias; ties to the lower index, NaN last. weights
    [tokens, top_k] = s at the picks, divided by their sum with `normalize`,
    times `scale`; scores [tokens, E], when given, = s. weights and scores
    share one dtype, the logits' or fp32 (sputnik_router_score_topk;
    sputnik/block/router.h). Type, shape, limit and aliasing errors are raised
    before the library is called."""
    what = "RouterScoreTopK"
    code, tokens, e, k, wcode = _router_head(
        logits, top_experts, weights, scores, what)
    if bias is not None:
        _router_stat(bias, logits, e, "bias")
    _router_groups(e, k, num_groups, topk_groups, what)
    scale = _router_scale(scale, what)
    _router_distinct([("top_experts", top_experts), ("weights", weights),
                      ("scores", scores)],
                     [("logits", logits), ("bias", bias)], what)
    _check(lib().sputnik_router_score_topk(
        _ptr(logits), _ptr(bias), _ptr(top_experts), _ptr(weights),
        _ptr(scores), tokens, e, k, num_groups, topk_groups,
        int(bool(normalize)), scale, code, wcode, _stream(stream)), what)


def RouterScoreTopKGrad(logits, top_experts, dweights, dlogits,  # noqa: N802
                        normalize=False, scale=1.0, dscores=None,
                        stream=None):
    """dlogits [tokens, E] (the logits' dtype): the gradient of
    RouterScoreTopK's weights (and scores, with `dscores`) with respect to
    the logits, the sigmoid recomputed from `logits`; `normalize` and `scale`
    as in the forward call. Bias and groups do not enter. A top_experts entry
    outside [0, E) contributes nothing, a duplicated one twice
    (sputnik_router_score_topk_grad). Errors are raised before the library is
    called."""
    what = "RouterScoreTopKGrad"
    code, tokens, e, k, wcode = _router_head(
        logits, top_experts, dweights, dscores, what, "d")
    _router_dlogits(dlogits, logits)
    scale = _router_scale(scale, what)
    _router_distinct([("dlogits", dlogits)],
                     [("logits", logits), ("top_experts", top_experts),
                      ("dweights", dweights), ("dscores", dscores)], what)
    _check(lib().sputnik_router_score_topk_grad(
        _ptr(logits), _ptr(top_experts), _ptr(dweights), _ptr(dscores),
        _ptr(dlogits), tokens, e, k, int(bool(normalize)), scale, code, wcode,
        _stream(stream)), what)


def _moe_sort_sizes(n, num_experts, what: str):
    n, e = int(n), int(num_experts)
    if n < 0 or not 1 <= e <= ROUTER_MAX_EXPERTS:
        raise ValueError(f"{what}: n = {n} must be >= 0 and num_experts = "
                         f"{e} in [1, {ROUTER_MAX_EXPERTS}]")
    if n + 127 * e > 2 ** 31 - 1:
        raise ValueError(f"{what}: n + 127 * num_experts passes INT_MAX")
    return n, e


def moe_sort_workspace_bytes(n: int, num_experts: int) -> int:
    """Bytes of workspace MoeSort needs for n assignments over num_experts:
    ceil(n / 1024) * (num_experts + 1) * 4
    (sputnik_moe_sort_workspace_bytes)."""
    n, e = _moe_sort_sizes(n, num_experts, "moe_sort_workspace_bytes")
    return int(lib().sputnik_moe_sort_workspace_bytes(n, e))


def MoeSort(top_experts, num_experts, rows, indices, bin_ids, bins,  # noqa: N802
            tokens_per_expert, padded_bins, row_of, workspace, stream=None):
    """The routing tensors of moe.h from top_experts (int32, n elements of
    any shape) in one call: a stable counting sort by expert into indices /
    bin_ids (int32 [n]), the counts as bins / tokens_per_expert / padded_bins
    (int32 [num_experts]) and row_of (int32 [n]) for a padded matrix of
    `rows` rows. `workspace`: a contiguous tensor of at least
    moe_sort_workspace_bytes(n, num_experts) bytes (None when that is 0); it
    needs no initialisation (sputnik_moe_sort). Type and shape errors are
    raised before the library is called."""
    _moe_meta(top_experts, None, "top_experts")
    n, e = _moe_sort_sizes(top_experts.numel(), num_experts, "MoeSort")
    for name, t in (("indices", indices), ("bin_ids", bin_ids),
                    ("row_of", row_of)):
        _moe_meta(t, n, name)
    for name, t in (("bins", bins), ("tokens_per_expert", tokens_per_expert),
                    ("padded_bins", padded_bins)):
        _moe_meta(t, e, name)
    if isinstance(rows, bool) or not isinstance(rows, int) or rows < 0 \
            or rows % 128:
        raise ValueError(f"MoeSort: {rows!r} padded rows, not a multiple of "
                         "128")
    need = (n + MOE_SORT_CHUNK - 1) // MOE_SORT_CHUNK * (e + 1) * 4
    have = _workspace_bytes(workspace, need, "MoeSort")
    _check(lib().sputnik_moe_sort(
        _ptr(top_experts), n, e, rows, _ptr(indices), _ptr(bin_ids),
        _ptr(bins), _ptr(tokens_per_expert), _ptr(padded_bins), _ptr(row_of),
        _ptr(workspace), have, _stream(stream)), "MoeSort")


def Bitmask(m: BlockMatrix, stream=None):  # noqa: N802
    """reference sputnik/block/bitmask/bitmask.h:10 (on the device): the
    BitMatrix of m's topology, over the transposed order when m.offsets_t is
    set (call AllocateBitmaskBuffers after AllocateTransposeBuffers then)."""
    cm = m._c()
    _check(lib().sputnik_bitmask(ctypes.byref(cm), _stream(stream)), "Bitmask")


def AllocateBitmaskBuffers(m: BlockMatrix):  # noqa: N802
    """reference bitmask.h:16-23 (uint64 words, torch-owned)."""
    import torch

    cm = m._c()
    words = lib().sputnik_bitmask_bytes(ctypes.byref(cm)) // 8
    m.bitmask = torch.empty(max(int(words), 1), dtype=torch.int64,
                            device=m.offsets.device)


def FreeBitmaskBuffers(m: BlockMatrix):  # noqa: N802
    m.bitmask = None


def sdd_plan(a, transpose_a, b, transpose_b, c) -> int:
    """SDD tile plan the dispatcher picks on the current device: 1 grouped
    128x512 tiles, 2 grouped tiles with each group's K split over 2-8
    workgroups, 0 one k-split block per workgroup, -1 rejected."""
    ca, cb, cc = a._c(), b._c(), c._c()
    return int(lib().sputnik_sdd_plan(ctypes.byref(ca), int(bool(transpose_a)),
                                      ctypes.byref(cb), int(bool(transpose_b)),
                                      ctypes.byref(cc)))


def sdd_kernel(a, transpose_a, b, transpose_b, c) -> int:
    """The kernel behind sdd_plan's tile plan: 0 8-wave k-split block tile,
    1 8-wave grouped, 2 4-wave K-split, 3 4-wave grouped, 4 B transposed
    into a library buffer then 4-wave grouped (NT / TT over a large B), -1
    rejected (sputnik_sdd_kernel)."""
    ca, cb, cc = a._c(), b._c(), c._c()
    return int(lib().sputnik_sdd_kernel(ctypes.byref(ca), int(bool(transpose_a)),
                                        ctypes.byref(cb), int(bool(transpose_b)),
                                        ctypes.byref(cc)))


def dds_plan(a, transpose_a, b, transpose_b, c, stream=None) -> int:
    """Kernel a DDS launch on `stream` would use: 0 8-wave tile, 1 4-wave
    kernel, 2 tall, 3 split (8-wave), -1 rejected (sputnik_dds_plan)."""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream().cuda_stream
    ca, cb, cc = a._c(), b._c(), c._c()
    return int(lib().sputnik_dds_plan(ctypes.byref(ca), int(bool(transpose_a)),
                                      ctypes.byref(cb), int(bool(transpose_b)),
                                      ctypes.byref(cc), ctypes.c_void_p(stream)))


def pair_errors() -> int:
    """Pair hand-offs since the last call whose consumer timed out (its
    output tile is NaN; sputnik_pair_errors() in include/sputnik_amd.h)."""
    return int(lib().sputnik_pair_errors())


def capture_workspaces() -> int:
    """Workspaces made for graph-captured launches on the current device
    (sputnik_capture_workspaces() in include/sputnik_amd.h)."""
    return int(lib().sputnik_capture_workspaces())


def build_hash() -> str:
    return lib().sputnik_build_hash().decode()


def AllocateTransposeBuffers(a: BlockMatrix):  # noqa: N802
    """reference arguments.h:233-245 (torch-owned device workspaces)."""
    import torch

    dev = a.offsets.device
    bcols = a.cols // AsInt(a.block_size)
    a.offsets_t = torch.empty(bcols + 1, dtype=torch.int32, device=dev)
    a.indices_t = torch.empty(a.num_blocks, dtype=torch.int16, device=dev)
    a.block_offsets = torch.empty(a.num_blocks, dtype=torch.int32, device=dev)


def FreeTransposeBuffers(a: BlockMatrix):  # noqa: N802
    a.offsets_t = a.indices_t = a.block_offsets = None


def AllocateRowIndicesBuffer(a: BlockMatrix):  # noqa: N802
    """reference arguments.h:259-263"""
    import torch

    a.row_indices = torch.empty(a.num_blocks, dtype=torch.int16,
                                device=a.offsets.device)


def FreeRowIndicesBuffer(a: BlockMatrix):  # noqa: N802
    a.row_indices = None


_OPS = {"dsd": 0, "dds": 1, "sdd": 2, "ssd": 3, "sds": 4, "dss": 5}


def can_implement(op: str, a, transpose_a, b, transpose_b, c) -> bool:
    """Host-only: would the library accept this problem? (no device work)"""
    ca, cb, cc = a._c(), b._c(), c._c()
    return bool(lib().sputnik_can_implement(
        _OPS[op], ctypes.byref(ca), int(bool(transpose_a)), ctypes.byref(cb),
        int(bool(transpose_b)), ctypes.byref(cc)))


def dsd_plan(a, transpose_a, b, transpose_b, c, stream=None) -> int:
    """Kernel a DSD launch on `stream` (torch's current stream by default)
    would use: 0 8-wave tile, 1 4-wave kernel, 2 tall, 3 split, 4 tall
    pipeline (4-wave, persistent), -1 rejected
    (sputnik_dsd_plan)."""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream().cuda_stream
    ca, cb, cc = a._c(), b._c(), c._c()
    return int(lib().sputnik_dsd_plan(ctypes.byref(ca), int(bool(transpose_a)),
                                      ctypes.byref(cb), int(bool(transpose_b)),
                                      ctypes.byref(cc), ctypes.c_void_p(stream)))


def select_dsd_kernel(four_wave: int = -1) -> int:
    """DSD / DDS / grouped-SDD kernel choice (sputnik_select_dsd_kernel): 1
    the 4-wave hand-scheduled kernel where it pays (default), 2-7 wherever
    it applies with a fixed variant (kEpi = mode - 2: 0 workgroup epilogue,
    1 per-wave, 2 specialized last block, 3 double slots, 4 double slots +
    barrier every other step + interleaved copy-out, 5 double slots +
    interleaved copy-out; transposed and SDD launches take the variant they
    have), 0 the 8-wave kernel, -1 query only. Returns the previous
    choice."""
    return int(lib().sputnik_select_dsd_kernel(int(four_wave)))


TUNING_UNKNOWN = -(2 ** 31)


def tuning(name: str, value: Optional[int] = None) -> int:
    """UNSUPPORTED tuning knob (sputnik_tuning_get / sputnik_tuning_set,
    include/sputnik_amd.h; tests and A/B experiments only): returns the
    knob's value, or with `value` sets it and returns the previous one.
    Raises KeyError for an unknown name or an out-of-range value."""
    L = lib()
    if value is None:
        v = int(L.sputnik_tuning_get(name.encode()))
    else:
        v = int(L.sputnik_tuning_set(name.encode(), int(value)))
    if v == TUNING_UNKNOWN:
        raise KeyError(f"tuning knob {name!r} (value {value!r})")
    return v


def version() -> str:
    return lib().sputnik_version().decode()


# Full-result gathers of a sharded product (host-side torch.distributed, off
# the hot path; sputnik_amd/gather.py).
from .gather import (allgather_concat, gather_block_runs,  # noqa: E402
                     gather_col_panels, gather_row_panels)


# ---- fp8 products (sputnik/block/fp8.h) --------------------------------------

def _fp8_buffer(t, dtype, shape, what: str) -> None:
    """A buffer of an fp8 call: `dtype`, `shape`, contiguous. Raises before
    any library call."""
    if getattr(t, "dtype", None) != dtype:
        raise TypeError(f"{what} is {getattr(t, 'dtype', None)}, expected "
                        f"{dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} has shape {tuple(t.shape)}, expected "
                         f"{tuple(shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")


def _fp8_tiles(n: int, what: str) -> int:
    if n % 128:
        raise ValueError(f"{what} = {n} is not a multiple of 128")
    return n // 128


def QuantizeRows(x, q, scales, pow2=False, activation=None, gate=None,  # noqa: N802
                 stream=None):
    """q (torch.float8_e4m3fn, x's shape) and scales (fp32 [rows, cols /
    128]) of x [rows, cols] (fp16 / bf16), one scale per 1 x 128 tile:
    scale = max(amax / 448, 2^-126), or with `pow2` the smallest power of two
    that keeps amax / scale <= 448; q = rne(x / scale) (sputnik_quantize_rows;
    sputnik/block/fp8.h has the format). With `activation` the rows of
    act(x), or with `gate` (x's shape and dtype) of x * act(gate), are
    quantised, each evaluated as BlockActivation / BlockGate evaluate it.
    Type and shape errors are raised before the library is called."""
    import torch

    _moe_matrix(x, None, None, "x")
    dtype = _dtype_code(x)
    rows, cols = int(x.shape[0]), int(x.shape[1])
    tiles = _fp8_tiles(cols, "QuantizeRows: cols")
    _fp8_buffer(q, torch.float8_e4m3fn, (rows, cols), "q")
    _fp8_buffer(scales, torch.float32, (rows, tiles), "scales")
    if gate is not None:
        if activation is None:
            raise ValueError("QuantizeRows: a gate needs its activation")
        _fp8_buffer(gate, x.dtype, (rows, cols), "gate")
    act = None if activation is None else _act_code(activation)
    L, p2, st = lib(), int(bool(pow2)), _stream(stream)
    if gate is not None:
        code = L.sputnik_quantize_rows_gated(
            _ptr(x), _ptr(gate), rows, cols, act, _ptr(q), _ptr(scales), p2,
            dtype, st)
    elif act is not None:
        code = L.sputnik_quantize_rows_act(
            _ptr(x), rows, cols, act, _ptr(q), _ptr(scales), p2, dtype, st)
    else:
        code = L.sputnik_quantize_rows(_ptr(x), rows, cols, _ptr(q),
                                       _ptr(scales), p2, dtype, st)
    _check(code, "QuantizeRows")


def QuantizeWeight(w, q, scales, transpose=False, pow2=False, stream=None):  # noqa: N802
    """q (torch.float8_e4m3fn [n, k], k-contiguous) and scales (fp32 [k / 128,
    n / 128], one per 128 x 128 block) of the weight w [k, n] (fp16 / bf16);
    with `transpose` the tensor passed holds w^T, [n, k]
    (sputnik_quantize_weight)."""
    import torch

    _moe_matrix(w, None, None, "w")
    k, n = int(w.shape[0]), int(w.shape[1])
    if transpose:
        k, n = n, k
    kb, nb = _fp8_tiles(k, "QuantizeWeight: k"), _fp8_tiles(n, "QuantizeWeight: n")
    _fp8_buffer(q, torch.float8_e4m3fn, (n, k), "q")
    _fp8_buffer(scales, torch.float32, (kb, nb), "scales")
    _check(lib().sputnik_quantize_weight(
        _ptr(w), k, n, int(bool(transpose)), _ptr(q), _ptr(scales),
        int(bool(pow2)), _dtype_code(w), _stream(stream)), "QuantizeWeight")


def _fp8_weight(bq, b_scales, what: str):
    """(n, k) of a quantised weight: bq e4m3 [n, k], b_scales fp32 [k / 128,
    n / 128]."""
    import torch

    if getattr(bq, "dtype", None) != torch.float8_e4m3fn or bq.dim() != 2:
        raise TypeError(f"{what}: bq must be a 2-D torch.float8_e4m3fn tensor")
    n, k = int(bq.shape[0]), int(bq.shape[1])
    _fp8_buffer(bq, torch.float8_e4m3fn, (n, k), "bq")
    _fp8_buffer(b_scales, torch.float32,
                (_fp8_tiles(k, f"{what}: k"), _fp8_tiles(n, f"{what}: n")),
                "b_scales")
    return n, k


FP8_ACCUMULATE = {"fp32": 0, "fast": 1}


def _fp8_accumulate(accumulate, what: str) -> int:
    """The Fp8Accumulate code of "fp32" / "fast"; raises before any library
    call."""
    if not isinstance(accumulate, str) or accumulate not in FP8_ACCUMULATE:
        raise ValueError(f"{what}: accumulate must be 'fp32' or 'fast', not "
                         f"{accumulate!r}")
    return FP8_ACCUMULATE[accumulate]


def SddFp8(aq, a_scales, bq, b_scales, c, stream=None,  # noqa: N802
           accumulate="fp32"):
    """C (BlockMatrix of fp16 / bf16 block values, with row_indices) = Aq .
    Bq at C's stored blocks: aq e4m3 [c.rows, k] with a_scales fp32 [c.rows,
    k / 128] (QuantizeRows), bq e4m3 [c.cols, k] with b_scales fp32 [k / 128,
    c.cols / 128] (QuantizeWeight). acc = fma(sa * sb, P, acc) per k-block
    in fp32, rounded once (sputnik_sdd_fp8). `accumulate`: "fp32" (P summed
    in fp32) or "fast" (P from the scaled e4m3 MFMA, Fp8Accumulate::kFast of
    sputnik/block/fp8.h; sputnik_sdd_fp8_acc)."""
    import torch

    mode = _fp8_accumulate(accumulate, "SddFp8")
    if not isinstance(c, BlockMatrix):
        raise TypeError("SddFp8 writes a BlockMatrix")
    n, k = _fp8_weight(bq, b_scales, "SddFp8")
    if n != c.cols:
        raise ValueError(f"SddFp8: bq has {n} rows, C {c.cols} columns")
    _fp8_buffer(aq, torch.float8_e4m3fn, (c.rows, k), "aq")
    _fp8_buffer(a_scales, torch.float32, (c.rows, k // 128), "a_scales")
    cc = c._c()
    if mode == 0:
        code = lib().sputnik_sdd_fp8(
            _ptr(aq), _ptr(a_scales), k, _ptr(bq), _ptr(b_scales),
            ctypes.byref(cc), _dtype_code(c.data), _stream(stream))
    else:
        code = lib().sputnik_sdd_fp8_acc(
            _ptr(aq), _ptr(a_scales), k, _ptr(bq), _ptr(b_scales),
            ctypes.byref(cc), _dtype_code(c.data), mode, _stream(stream))
    _check(code, "SddFp8")


def DsdFp8(s, s_scales, bq, b_scales, c, stream=None,  # noqa: N802
           accumulate="fp32"):
    """C (Matrix of fp16 / bf16, [s.rows, n]) = Sq . Bq: s a BlockMatrix whose
    data holds e4m3 block values with s_scales fp32 [blocks * 128], one per
    row of each stored block in storage order (QuantizeRows over the block
    values as [blocks * 128, 128]); bq / b_scales as SddFp8, k = s.cols. A
    block row without blocks gives +0 rows (sputnik_dsd_fp8). `accumulate`
    as SddFp8 (sputnik_dsd_fp8_acc)."""
    import torch

    mode = _fp8_accumulate(accumulate, "DsdFp8")
    if not isinstance(s, BlockMatrix) or not isinstance(c, Matrix):
        raise TypeError("DsdFp8 takes a BlockMatrix and writes a Matrix")
    n, k = _fp8_weight(bq, b_scales, "DsdFp8")
    if k != s.cols or n != c.cols or c.rows != s.rows:
        raise ValueError(f"DsdFp8 shapes [{s.rows}, {s.cols}] x [{k}, {n}] "
                         f"-> [{c.rows}, {c.cols}]")
    if getattr(s.data, "dtype", None) != torch.float8_e4m3fn:
        raise TypeError("DsdFp8: s.data must be torch.float8_e4m3fn")
    _fp8_buffer(s_scales, torch.float32, (s.num_blocks * 128,), "s_scales")
    cs, cc = s._c(), c._c()
    if mode == 0:
        code = lib().sputnik_dsd_fp8(
            ctypes.byref(cs), _ptr(s_scales), _ptr(bq), _ptr(b_scales),
            ctypes.byref(cc), _dtype_code(c.data), _stream(stream))
    else:
        code = lib().sputnik_dsd_fp8_acc(
            ctypes.byref(cs), _ptr(s_scales), _ptr(bq), _ptr(b_scales),
            ctypes.byref(cc), _dtype_code(c.data), mode, _stream(stream))
    _check(code, "DsdFp8")


def Fp8IntervalSums(aq, bq, p, accumulate="fp32", stream=None):  # noqa: N802
    """P (fp32 [k / 128, m, n]) of aq e4m3 [m, k] and bq e4m3 [n, k]: per
    k-block the interval sum from +0 as SddFp8 / DsdFp8 form it under
    `accumulate` ("fp32" or "fast"). The definition of P in
    sputnik/block/fp8.h as a callable; a cold kernel
    (sputnik_fp8_interval_sums)."""
    import torch

    mode = _fp8_accumulate(accumulate, "Fp8IntervalSums")
    if getattr(aq, "dtype", None) != torch.float8_e4m3fn or aq.dim() != 2:
        raise TypeError("Fp8IntervalSums: aq must be a 2-D "
                        "torch.float8_e4m3fn tensor")
    m, k = int(aq.shape[0]), int(aq.shape[1])
    if getattr(bq, "dtype", None) != torch.float8_e4m3fn or bq.dim() != 2:
        raise TypeError("Fp8IntervalSums: bq must be a 2-D "
                        "torch.float8_e4m3fn tensor")
    n = int(bq.shape[0])
    _fp8_tiles(m, "Fp8IntervalSums: m")
    _fp8_tiles(n, "Fp8IntervalSums: n")
    kb = _fp8_tiles(k, "Fp8IntervalSums: k")
    _fp8_buffer(aq, torch.float8_e4m3fn, (m, k), "aq")
    _fp8_buffer(bq, torch.float8_e4m3fn, (n, k), "bq")
    _fp8_buffer(p, torch.float32, (kb, m, n), "p")
    _check(lib().sputnik_fp8_interval_sums(
        _ptr(aq), _ptr(bq), m, n, k, mode, _ptr(p), _stream(stream)),
        "Fp8IntervalSums")


FP8_STAGES = {None: 0, "act": 1, "act_grad": 2}


def _fp8_pair(q, scales, q_shape, s_shape, what: str):
    """An output pair of a tile quantiser: both given or both None."""
    import torch

    if (q is None) != (scales is None):
        raise ValueError(f"{what}: an output pair is given whole or not at "
                         "all")
    if q is not None:
        _fp8_buffer(q, torch.float8_e4m3fn, q_shape, f"{what} bytes")
        _fp8_buffer(scales, torch.float32, s_shape, f"{what} scales")
    return _ptr(q) if q is not None else None, (
        _ptr(scales) if scales is not None else None)


def QuantizeTiles(x, q=None, scales=None, qt=None, scales_t=None,  # noqa: N802
                  pow2=False, stream=None):
    """x [rows, cols] (fp16 / bf16, both multiples of 128) quantised along
    either axis or both, read once: the row pair q [rows, cols], scales
    [rows, cols / 128] is QuantizeRows' bit for bit; the column pair qt
    (e4m3 [cols, rows]) and scales_t (fp32 [rows / 128, cols]) has one scale
    per 128 x 1 column tile (sputnik_quantize_tiles)."""
    _moe_matrix(x, None, None, "x")
    rows, cols = int(x.shape[0]), int(x.shape[1])
    rt = _fp8_tiles(rows, "QuantizeTiles: rows")
    ct = _fp8_tiles(cols, "QuantizeTiles: cols")
    pq, ps = _fp8_pair(q, scales, (rows, cols), (rows, ct), "QuantizeTiles: row")
    pt, pst = _fp8_pair(qt, scales_t, (cols, rows), (rt, cols),
                        "QuantizeTiles: column")
    if q is None and qt is None:
        raise ValueError("QuantizeTiles: no output")
    _check(lib().sputnik_quantize_tiles(
        _ptr(x), rows, cols, pq, ps, pt, pst, int(bool(pow2)), _dtype_code(x),
        _stream(stream)), "QuantizeTiles")


def QuantizeBlocks(s, q=None, scales=None, qt=None, scales_t=None,  # noqa: N802
                   stage=None, activation=None, z=None, pow2=False,
                   stream=None):
    """The block values of the BlockMatrix s (fp16 / bf16) after `stage`
    (None; "act": act(x); "act_grad": x * act'(z), z block values like
    s.data), quantised along either axis or both: the row pair q [blocks,
    128, 128], scales [blocks * 128] in storage order, as QuantizeRows over
    the same values; the column pair in the transposed order, output block j
    being source block s.block_offsets[j] stored transposed, with scales_t
    [blocks * 128] per source column (sputnik_quantize_blocks)."""
    import torch

    if not isinstance(s, BlockMatrix):
        raise TypeError("QuantizeBlocks takes a BlockMatrix")
    if stage not in FP8_STAGES:
        raise ValueError(f"QuantizeBlocks: stage must be one of "
                         f"{list(FP8_STAGES)}")
    nb = s.num_blocks
    if s.data.dtype not in (torch.float16, torch.bfloat16):
        raise TypeError("QuantizeBlocks: s.data must be fp16 / bf16")
    act = 0 if stage is None else _act_code(activation)
    if stage == "act_grad":
        _fp8_buffer(z, s.data.dtype, tuple(s.data.shape), "z")
    pq, ps = _fp8_pair(q, scales, (nb, 128, 128), (nb * 128,),
                       "QuantizeBlocks: row")
    pt, pst = _fp8_pair(qt, scales_t, (nb, 128, 128), (nb * 128,),
                        "QuantizeBlocks: column")
    if q is None and qt is None:
        raise ValueError("QuantizeBlocks: no output")
    cs = s._c()
    _check(lib().sputnik_quantize_blocks(
        ctypes.byref(cs), FP8_STAGES[stage], act,
        _ptr(z) if stage == "act_grad" else None, pq, ps, pt, pst,
        int(bool(pow2)), _dtype_code(s.data), _stream(stream)),
        "QuantizeBlocks")


def TransposeWeightFp8(q, scales, qt, scales_t, stream=None):  # noqa: N802
    """qt (e4m3 [k, n]) and scales_t (fp32 [n / 128, k / 128]) of a quantised
    weight q [n, k], scales [k / 128, n / 128]: the byte transpose, which is
    QuantizeWeight of the transposed weight bit for bit
    (sputnik_fp8_transpose_weight)."""
    import torch

    n, k = _fp8_weight(q, scales, "TransposeWeightFp8")
    _fp8_buffer(qt, torch.float8_e4m3fn, (k, n), "qt")
    _fp8_buffer(scales_t, torch.float32, (n // 128, k // 128), "scales_t")
    _check(lib().sputnik_fp8_transpose_weight(
        _ptr(q), _ptr(scales), k, n, _ptr(qt), _ptr(scales_t),
        _stream(stream)), "TransposeWeightFp8")


def DsdFp8Wgrad(s, s_scales, bq, b_scales, c, add=False,  # noqa: N802
                accumulate="fp32", stream=None):
    """C (Matrix [s.rows, n] of fp16 / bf16 / fp32) = Sq . Bq as DsdFp8 with
    b_scales fp32 [s.cols / 128, n], one per k-block and output column
    (QuantizeTiles' scales_t): acc = fma(sa[row] * sb[kb, col], P, acc). With
    `add` C = round(acc + float(C)) and block rows of s without blocks are
    left untouched. `dtype` is the 16-bit type: C's, or with an fp32 C
    irrelevant to the result (sputnik_dsd_fp8_wgrad)."""
    import torch

    mode = _fp8_accumulate(accumulate, "DsdFp8Wgrad")
    if not isinstance(s, BlockMatrix) or not isinstance(c, Matrix):
        raise TypeError("DsdFp8Wgrad takes a BlockMatrix and writes a Matrix")
    if getattr(bq, "dtype", None) != torch.float8_e4m3fn or bq.dim() != 2:
        raise TypeError("DsdFp8Wgrad: bq must be a 2-D torch.float8_e4m3fn "
                        "tensor")
    n, k = int(bq.shape[0]), int(bq.shape[1])
    _fp8_tiles(n, "DsdFp8Wgrad: n")
    kb = _fp8_tiles(k, "DsdFp8Wgrad: k")
    _fp8_buffer(bq, torch.float8_e4m3fn, (n, k), "bq")
    _fp8_buffer(b_scales, torch.float32, (kb, n), "b_scales")
    if k != s.cols or n != c.cols or c.rows != s.rows:
        raise ValueError(f"DsdFp8Wgrad shapes [{s.rows}, {s.cols}] x [{k}, "
                         f"{n}] -> [{c.rows}, {c.cols}]")
    if getattr(s.data, "dtype", None) != torch.float8_e4m3fn:
        raise TypeError("DsdFp8Wgrad: s.data must be torch.float8_e4m3fn")
    _fp8_buffer(s_scales, torch.float32, (s.num_blocks * 128,), "s_scales")
    f32 = c.data.dtype == torch.float32
    cs, cc = s._c(), c._c()
    _check(lib().sputnik_dsd_fp8_wgrad(
        ctypes.byref(cs), _ptr(s_scales), _ptr(bq), _ptr(b_scales),
        ctypes.byref(cc), 0 if f32 else _dtype_code(c.data), int(f32),
        int(bool(add)), mode, _stream(stream)), "DsdFp8Wgrad")


__all__ = [
    "AllocateBitmaskBuffers", "AllocateRowIndicesBuffer",
    "AllocateTransposeBuffers", "AsInt", "Bitmask", "FreeBitmaskBuffers",
    "build_hash", "capture_workspaces", "pair_errors", "sdd_plan", "sdd_kernel",
    "dds_plan",
    "select_dsd_kernel", "dsd_plan", "tuning",
    "set_stream_workspace", "sdd_workspace_bytes", "dsd_workspace_bytes",
    "retained_bytes", "release_workspaces", "incall_events", "bt_launches",
    "BlockMatrix", "BlockSize", "ExpertTopology", "FreeRowIndicesBuffer",
    "MaskToBcsr",
    "FreeTransposeBuffers", "Matmul", "MatmulEx", "Matrix", "RowIndices",
    "MatmulAccumulate", "MatmulAccumulateEx",
    "MatmulActivation", "MatmulActivationGrad", "BlockActivation",
    "BlockActivationGrad", "SPUTNIK_ACT_RELU", "SPUTNIK_ACT_GELU",
    "SPUTNIK_ACT_SILU", "sdd_act_route",
    "MatmulGated", "MatmulGatedGrad", "BlockGate", "BlockGateGrad",
    "MatmulBias", "MatmulBiasActivation", "MatmulBiasGated", "BlockColumnSum",
    "QuantizeRows", "QuantizeWeight", "SddFp8", "DsdFp8", "Fp8IntervalSums",
    "FP8_ACCUMULATE", "QuantizeTiles", "QuantizeBlocks", "TransposeWeightFp8",
    "DsdFp8Wgrad", "FP8_STAGES",
    "PaddedScatterBias", "PaddedScatterBiasWeightGrad",
    "PaddedScatterBiasGrad",
    "MoeBins", "MoeRowMap", "PaddedGather", "PaddedScatter",
    "PaddedScatterWeightGrad", "SPUTNIK_WEIGHTS_OPERAND",
    "SPUTNIK_WEIGHTS_F32",
    "RouterTopK", "RouterTopKGrad", "MoeSort", "moe_sort_workspace_bytes",
    "SPUTNIK_ROUTER_F16", "SPUTNIK_ROUTER_BF16", "SPUTNIK_ROUTER_F32",
    "MOE_SORT_CHUNK",
    "RouterTopKAux", "RouterTopKAuxGrad", "router_aux_workspace_bytes",
    "ROUTER_AUX_TOKENS",
    "RouterScoreTopK", "RouterScoreTopKGrad", "ROUTER_MAX_GROUPS",
    "SputnikError", "Transpose", "can_implement", "lib", "version",
    "allgather_concat", "gather_row_panels", "gather_col_panels",
    "gather_block_runs",
]
