"""GAMLP's learnable hop attention on the device (LearnableWeightedMessageOp, combination types gate /
ori_ref / jk): srg_hop_scores_f32 + srg_hop_attend_f32 forward, srg_hop_attend_grad_f32 +
srg_hop_scores_grad_f32 backward, without the [H*n, (T+1)*d] panel of the torch composition
(DESIGN.md §5.4.2); and the recursive attention (IterateLearnableWeightedMessageOp, combination type
recursive): srg_hop_recur_scores_f32 + srg_hop_recur_attend_f32 forward, srg_hop_recur_attend_grad_f32 +
srg_hop_recur_scores_grad_f32 backward, a scalar recurrence per row between two streaming passes instead of
the composition's H^2 panel-sized steps.  The hop panels are precomputed constants:
gradients go to the weight and the bias.  With `index=` both attend over a mini-batch of rows of the panels
through the srg_hop_*_rows_f32 entries, which read row index[r] where the others read row r: no gathered
[B, d] copies of the hops.
"""
from __future__ import annotations

import ctypes

import torch
from torch.autograd.function import once_differentiable

from srgnn import _lib

KINDS = {"gate": _lib.SRG_HOP_GATE, "ori_ref": _lib.SRG_HOP_ORI_REF, "jk": _lib.SRG_HOP_JK}


def in_dim(kind: str, T: int, d: int) -> int:
    """Input width of the operator's Linear for a list of T hops of d columns."""
    return {"gate": d, "ori_ref": 2 * d, "jk": T * d + d, "recursive": 2 * d}[kind]


def _pairing(kind: str) -> int:
    # the reference transposes gate's scores and .view(-1, H)s the hop-major vector of the other two
    return _lib.SRG_HOP_PAIR_TRANSPOSE if kind == "gate" else _lib.SRG_HOP_PAIR_FLAT


def _panel_args(feats):
    T = len(feats)
    ptrs = (ctypes.c_void_p * T)(*[f.data_ptr() for f in feats])
    lds = (ctypes.c_int64 * T)(*[f.stride(0) if f.shape[0] > 1 else f.shape[1] for f in feats])
    return ptrs, lds


def _call(dev, name, ptrs, lds, index, n_src, *rest):
    """The entry `name` on whole panels (index None), or its row-indexed twin on the rows `index` names."""
    if index is None:
        _lib.call(dev, name, ptrs, lds, *rest)
    else:
        _lib.call(dev, name.replace("_f32", "_rows_f32"), ptrs, lds, index.data_ptr(), n_src, *rest)


def _index(index, feat_list, check):
    """The batch rows as a contiguous int64 tensor on the panels' device.  check: one aminmax and its host sync;
    an index outside [-n, n) raises IndexError, negative ones are wrapped as torch wraps them.  Without it the
    index goes to the kernels as it is, where an index outside [0, n) reads as a row of zeros."""
    if index is None:
        return None
    index = torch.as_tensor(index)
    if index.dim() != 1 or index.dtype.is_floating_point or index.dtype.is_complex or index.dtype == torch.bool:
        raise TypeError(f"hop_attention: index must be a 1-d integer tensor, got {index.dtype} {tuple(index.shape)}")
    n = feat_list[0].shape[0]
    index = index.to(device=feat_list[0].device, dtype=torch.int64).contiguous()
    if check and index.numel() > 0:
        lo, hi = (int(v) for v in torch.aminmax(index))
        if lo < -n or hi >= n:
            raise IndexError(f"hop_attention: index {lo if lo < -n else hi} is out of bounds for hops of {n} rows")
        if lo < 0:
            index = torch.where(index < 0, index + n, index)
    return index


def _check(feat_list, start, end, kind, weight, bias, kinds=KINDS):
    if kind not in kinds:
        raise ValueError(f"hop_attention: kind {kind!r} is not one of {sorted(kinds)}")
    if not isinstance(feat_list, (list, tuple)) or len(feat_list) == 0:
        raise ValueError("hop_attention: feat_list must be a non-empty list of hop tensors")
    T = len(feat_list)
    if T > _lib.SRG_HOP_MAX:
        raise ValueError(f"hop_attention: {T} hop tensors, at most {_lib.SRG_HOP_MAX}")
    start, end = 0 if start is None else int(start), T if end is None else int(end)
    H = end - start
    if start < 0 or H < 1 or end > T:
        # the reference sizes its score matrix by end - start: a slice the list cannot fill is an error there too
        raise ValueError(f"hop_attention: hop slice [{start}, {end}) of {T} hops")
    if H > _lib.SRG_HOP_MAX:
        raise ValueError(f"hop_attention: {H} hops in the slice, at most {_lib.SRG_HOP_MAX}")
    f0 = feat_list[0]
    for k, f in enumerate(feat_list):
        if not isinstance(f, torch.Tensor) or f.dim() != 2:
            raise ValueError(f"hop_attention: hop {k} is not a 2-d tensor")
        if f.requires_grad:
            raise ValueError(f"hop_attention: hop {k} requires grad; the fused path treats the hops as constants")
        if f.dtype != torch.float32:
            raise TypeError(f"hop_attention: hop {k} is {f.dtype}, the fused path computes in float32")
        if not f.is_cuda:
            raise ValueError(f"hop_attention: hop {k} is on {f.device}, not on a HIP device")
        if f.shape != f0.shape or f.device != f0.device:
            raise ValueError(f"hop_attention: hop {k} is {tuple(f.shape)} on {f.device}, hop 0 "
                             f"{tuple(f0.shape)} on {f0.device}")
        if f.shape[1] < 1 or f.stride(1) != 1:
            raise ValueError(f"hop_attention: hop {k} needs >= 1 column and unit column stride")
    want = in_dim(kind, T, f0.shape[1])
    if weight.numel() != want or bias.numel() != 1:
        raise ValueError(f"hop_attention: {kind} over {T} hops of {f0.shape[1]} columns needs a weight of "
                         f"{want} elements and one bias, got {weight.numel()} and {bias.numel()}")
    for name, p in (("weight", weight), ("bias", bias)):
        if p.dtype != torch.float32 or p.device != f0.device:
            raise TypeError(f"hop_attention: {name} is {p.dtype} on {p.device}, the hops float32 on {f0.device}")
    return start, end


def _batch(feats, index):
    """(dev, n_src, d, n): the panels' device, rows and columns, and the rows attended over."""
    n_src, d = feats[0].shape
    return feats[0].device, n_src, d, n_src if index is None else index.numel()


def _grad_operand(grad, n, d):
    """(G, ldg): grad as float32 rows of unit column stride, as it is where it already is that."""
    G = grad if grad.dtype == torch.float32 and grad.stride(1) == 1 and (n <= 1 or grad.stride(0) >= d) \
        else grad.to(torch.float32).contiguous()
    return G, G.stride(0) if n > 1 else d


def _param_grads(dev, width, wants, query, *shape):
    """(dw, db, nbytes): the wanted gradients' buffers (None for the other) and the size `query` gives for the
    parameter gradient's scratch at `shape`."""
    dw = torch.empty(width, dtype=torch.float32, device=dev) if wants[0] else None
    db = torch.empty(1, dtype=torch.float32, device=dev) if wants[1] else None
    nbytes = ctypes.c_int64(0)
    _lib.check(_lib.query(query, *shape, ctypes.byref(nbytes)), query)
    return dw, db, nbytes.value


def _grads(dw, db, w_shape, b_shape, n_rest):
    """backward's tuple: the weight's and the bias's gradient, None for each of the n_rest other inputs."""
    return (None if dw is None else dw.view(w_shape), None if db is None else db.view(b_shape)) + (None,) * n_rest


class _HopAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, bias, start, end, kind, index, *feats):
        dev, n_src, d, n = _batch(feats, index)
        T, H = len(feats), end - start
        w, b = weight.detach().contiguous().view(-1), bias.detach().contiguous().view(-1)
        ptrs, lds = _panel_args(feats)
        zflat = torch.empty(H * n, dtype=torch.float32, device=dev)
        P = torch.empty((n, H), dtype=torch.float32, device=dev)
        out = torch.empty((n, d), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = _lib.stream(dev)
            _call(dev, "srg_hop_scores_f32", ptrs, lds, index, n_src, T, start, end, KINDS[kind], w.data_ptr(),
                  b.data_ptr(), zflat.data_ptr(), n, d, st)
            _call(dev, "srg_hop_attend_f32", ptrs, lds, index, n_src, T, start, end, zflat.data_ptr(), _pairing(kind),
                  P.data_ptr(), out.data_ptr(), d, n, d, st)
        ctx.save_for_backward(P, zflat, index, *feats)     # the panels by reference: no copy
        ctx.meta = (start, end, kind, weight.shape, bias.shape)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        P, zflat, index, *feats = ctx.saved_tensors
        start, end, kind, w_shape, b_shape = ctx.meta
        wants = ctx.needs_input_grad[:2]
        if not any(wants):
            return _grads(None, None, w_shape, b_shape, 4 + len(feats))
        dev, n_src, d, n = _batch(feats, index)
        T, H = len(feats), end - start
        G, ldg = _grad_operand(grad, n, d)
        ptrs, lds = _panel_args(feats)
        dP = torch.empty((n, H), dtype=torch.float32, device=dev)
        dz = torch.empty(H * n, dtype=torch.float32, device=dev)
        dw, db, nbytes = _param_grads(dev, in_dim(kind, T, d), wants, "srg_hop_scores_grad_scratch_bytes", n, d, T, H,
                                      KINDS[kind])
        with torch.cuda.device(dev):
            st = _lib.stream(dev)
            _call(dev, "srg_hop_attend_grad_f32", ptrs, lds, index, n_src, T, start, end, G.data_ptr(), ldg,
                  zflat.data_ptr(), P.data_ptr(), _pairing(kind), dP.data_ptr(), dz.data_ptr(), n, d, st)
            del dP
            scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
            _call(dev, "srg_hop_scores_grad_f32", ptrs, lds, index, n_src, T, start, end, KINDS[kind], dz.data_ptr(),
                  dw.data_ptr() if wants[0] else None, db.data_ptr() if wants[1] else None, scratch.data_ptr(),
                  n, d, st)
        return _grads(dw, db, w_shape, b_shape, 4 + len(feats))


def hop_attention(feat_list, start, end, kind, weight, bias, index=None, check=True):
    """out[i] = sum_h P[i, h] * feat_list[start + h][i] with P the reference's softmax(sigmoid(scores))
    (LearnableWeightedMessageOp's gate / ori_ref / jk), differentiable once in `weight` ([1, in_dim]) and
    `bias` ([1]).  feat_list: float32 [n, d] tensors on one HIP device, none requiring grad (row strides
    are free: column windows of wider panels pass as they are).  Raises if a fused kernel cannot run.

    index (a 1-d integer tensor of B batch rows, any order, duplicates allowed): the attention over the rows
    feat[index] of every hop, out [B, d], with the bits of hop_attention([f[index] for f in feat_list], ...)
    on contiguous copies of the same alignment, without making the copies; it gets no gradient.  check=True
    validates it with one aminmax and its host sync: outside [-n, n) raises IndexError before any launch,
    negative indices wrap as in torch.  check=False skips that (a loader whose indices were validated once):
    an index outside [0, n) then reads as a row of zeros."""
    start, end = _check(feat_list, start, end, kind, weight, bias)
    index = _index(index, feat_list, check)
    return _HopAttention.apply(weight, bias, start, end, kind, index, *feat_list)


class _HopAttentionRecursive(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, bias, end, index, *feats):
        dev, n_src, d, n = _batch(feats, index)
        T, H = len(feats), end
        w, b = weight.detach().contiguous().view(-1), bias.detach().contiguous().view(-1)
        ptrs, lds = _panel_args(feats)
        zp = torch.empty(H * n, dtype=torch.float32, device=dev)
        zq = torch.empty(H * n, dtype=torch.float32, device=dev)
        work = torch.empty((H * (H + 1) // 2 + H) * n, dtype=torch.float32, device=dev)
        P = torch.empty((n, H), dtype=torch.float32, device=dev)
        out = torch.empty((n, d), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = _lib.stream(dev)
            _call(dev, "srg_hop_recur_scores_f32", ptrs, lds, index, n_src, T, end, w.data_ptr(), zp.data_ptr(),
                  zq.data_ptr(), n, d, st)
            _call(dev, "srg_hop_recur_attend_f32", ptrs, lds, index, n_src, T, end, zp.data_ptr(), zq.data_ptr(),
                  b.data_ptr(), work.data_ptr(), P.data_ptr(), out.data_ptr(), d, n, d, st)
        ctx.save_for_backward(zq, work, index, *feats)     # the panels by reference: no copy
        ctx.meta = (end, weight.shape, bias.shape)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        zq, work, index, *feats = ctx.saved_tensors
        end, w_shape, b_shape = ctx.meta
        wants = ctx.needs_input_grad[:2]
        if not any(wants):
            return _grads(None, None, w_shape, b_shape, 2 + len(feats))
        dev, n_src, d, n = _batch(feats, index)
        T, H = len(feats), end
        G, ldg = _grad_operand(grad, n, d)
        ptrs, lds = _panel_args(feats)
        dzp = torch.empty(H * n, dtype=torch.float32, device=dev)
        dzq = torch.empty(H * n, dtype=torch.float32, device=dev)
        dw, db, nbytes = _param_grads(dev, 2 * d, wants, "srg_hop_recur_scores_grad_scratch_bytes", n, d, H)
        with torch.cuda.device(dev):
            st = _lib.stream(dev)
            _call(dev, "srg_hop_recur_attend_grad_f32", ptrs, lds, index, n_src, T, end, G.data_ptr(), ldg,
                  zq.data_ptr(), work.data_ptr(), dzp.data_ptr(), dzq.data_ptr(), n, d, st)
            scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
            _call(dev, "srg_hop_recur_scores_grad_f32", ptrs, lds, index, n_src, T, end, dzp.data_ptr(), dzq.data_ptr(),
                  dw.data_ptr() if wants[0] else None, db.data_ptr() if wants[1] else None, scratch.data_ptr(),
                  n, d, st)
        return _grads(dw, db, w_shape, b_shape, 2 + len(feats))


def hop_attention_recursive(feat_list, end, weight, bias, index=None, check=True):
    """The reference's recursive hop attention over feat_list[0 : end] (IterateLearnableWeightedMessageOp with
    start == 0, the only start it works with; later hops are ignored): hop i's per-node weight is
    sigmoid(Linear(2d, 1)([hop i | the combination so far])), the weights so far are re-softmaxed, and out is
    the combination under the last weights.  Differentiable once in `weight` ([1, 2d]) and `bias` ([1]).
    feat_list, index and check as for hop_attention.  Raises if a fused kernel cannot run."""
    _, end = _check(feat_list, 0, end, "recursive", weight, bias, kinds=("recursive",))
    index = _index(index, feat_list, check)
    return _HopAttentionRecursive.apply(weight, bias, end, index, *feat_list)
