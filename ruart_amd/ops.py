"""autograd wrappers around the SDNet kernels of libruart_hip.so (fp32, device tensors only).

Each Function's forward AND backward launch hand-written HIP kernels through the C ABI - the dense projections included
(``mm`` / ``linear`` / ``addmm`` on ruart_gemm_x3).  No library GEMM runs inside a training or inference step of the default
modes: the vendor library's solutions for these shapes are all stream-K kernels (Tensile ``SK3``: a fixed grid of workgroups that
exchange partial tiles through flags in memory and spin on each other), which need every workgroup of the launch resident at the
same time; three of them launched on three streams beside the encoder's 256-workgroup GEMMs do not get that, and the device stops
making progress (the hang of round 1).  Only the exact-fp32 validation mode (``use_trunk_mode(gemm="fp32")``) still calls
torch.mm, and SDNet runs that mode on ONE stream.
There is no CPU path: a CPU tensor raises ``hip.HipError``.
"""
import contextlib
import ctypes
import dataclasses
import os
import sys

import torch

from . import hip

_WS = {}
_PLAN_BYTES = {}      # (M, N, K, a K-contiguous, b K-contiguous) -> split-K workspace bytes of ruart_gemm_x3_plan


def _scratch(device, n, tag=""):
    key = (device, hip.stream_handle(device), tag)      # per stream: branches run concurrently
    t = _WS.get(key)
    if t is None or t.numel() < n:
        t = torch.empty(max(n, 4096), dtype=torch.float32, device=device)
        _WS[key] = t
    return t


class _NanFlag:
    """Device-side flag honouring the reference's NaN asserts (Models/Layers.py:169,290,430,462,467) with ONE
    host sync per step instead of one per op."""

    def __init__(self):
        self.flag = None

    def ensure(self, device):
        if self.flag is None or self.flag.device != device:
            self.flag = torch.zeros(1, dtype=torch.int32, device=device)
            hip.kernels().ruart_set_nan_flag(self.flag)
        return self.flag

    def check_and_clear(self):
        if self.flag is None:
            return
        bad = int(self.flag.item())
        self.flag.zero_()
        assert bad == 0, "NaN produced inside the SDNet kernels (reference: assert torch.sum(torch.isnan(x)) == 0)"


nan_flag = _NanFlag()


# ---------------------------------------------------------------------------------------------------------
ATTN_PANEL_MAX_L2 = 384           # key sets up to here: the whole-panel kernels (csrc/sdnet_attention.hip); above, up to 1024: the
                                  # key-block kernels (csrc/sdnet_attention_wide.hip).  Each entry point refuses the other's range.


class _FusedAttention(torch.autograd.Function):
    """out = softmax_j(mask(a . k^T)) . v with a = act(pa) * diag, k = act(pk)   (Models/Layers.py:228-231, 244, 275-288)."""

    @staticmethod
    def forward(ctx, pa, pk, v, mask, diag, relu, pscale=None):
        lib = hip.kernels()
        for t in (pa, pk, v):
            hip.require_gpu(t, torch.float32)
        nan_flag.ensure(pa.device)
        B, L1, h = pa.shape
        L2, D3 = pk.shape[1], v.shape[2]
        dl = 0 if diag is None else diag.numel()
        out = torch.empty(B, L1, D3, dtype=torch.float32, device=pa.device)
        probs = torch.empty(B, L1, L2, dtype=torch.float32, device=pa.device)
        fwd = lib.ruart_attn_fwd_wide if L2 > ATTN_PANEL_MAX_L2 else lib.ruart_attn_fwd_pscale
        fwd(pa, pk, v, mask, diag, dl, int(relu), pscale, out, probs, B, L1, L2, h, D3, hip.stream_ptr())
        ctx.save_for_backward(pa, pk, v, probs, diag, pscale)
        ctx.relu = int(relu)
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = hip.kernels()
        pa, pk, v, probs, diag, pscale = ctx.saved_tensors
        B, L1, h = pa.shape
        L2, D3 = pk.shape[1], v.shape[2]
        dl = 0 if diag is None else diag.numel()
        gout = gout.contiguous()
        ga, gk, gv = torch.empty_like(pa), torch.empty_like(pk), torch.empty_like(v)
        ds = torch.empty_like(probs)
        kdiag = diag
        if dl == 1 and ctx.needs_input_grad[4]:
            # a trainable scalar diag (the model's own is frozen): the kernels return grad_diag partials per column for a vector diag
            # only, so the backward runs with the scalar spread over the h columns - the same products, hence the same bits in every other
            # gradient - and the scalar's gradient is the sum of the column gradients
            if h == 1:
                raise hip.HipError("fused_attention: no gradient for a scalar diag with h == 1 (a one-column diag is the scalar form)")
            kdiag, dl = diag.reshape(1).expand(h).contiguous(), h
        gdiag = (torch.empty(B * ((L1 + 15) // 16), h, dtype=torch.float32, device=pa.device)
                 if (dl > 1 and ctx.needs_input_grad[4]) else None)
        bwd = lib.ruart_attn_bwd_wide if L2 > ATTN_PANEL_MAX_L2 else lib.ruart_attn_bwd_pscale
        bwd(pa, pk, v, probs, gout, kdiag, dl, ctx.relu, pscale, ga, gk, gv, gdiag, ds, B, L1, L2, h, D3, hip.stream_ptr())
        if gdiag is None:
            return ga, gk, gv, None, None, None, None
        gd = colsum(gdiag)
        return ga, gk, gv, None, (gd if kdiag is diag else gd.sum()).view_as(diag), None, None


def fused_attention(a, k, v, mask, diag=None, relu=False, prob_scale=None):
    """a (B,L1,h), k (B,L2,h), v (B,L2,D3) fp32; mask (B,L2) uint8/bool (0 = masked key).  With ``relu`` / ``diag`` the
    activation of the reference's AttentionScore is applied inside the kernel: a <- ReLU(a) * diag, k <- ReLU(k).
    ``prob_scale`` (B,L1,L2) fp32 of 0 / 1/(1-p): dropout on the attention probabilities (BERT).
    1 <= L2 <= 1024: up to 384 keys run ruart_attn_fwd_pscale / _bwd_pscale, 385 .. 1024 ruart_attn_fwd_wide / _bwd_wide; more keys
    raise ``HipError``."""
    m = mask.to(torch.uint8).contiguous()
    d = None if diag is None else diag.contiguous().view(-1)
    ps = None if prob_scale is None else prob_scale.contiguous()
    return _FusedAttention.apply(a.contiguous(), k.contiguous(), v.contiguous(), m, d, relu, ps)


# ---------------------------------------------------------------------------------------------------------
class _FusedScorer(torch.autograd.Function):
    """probs (B, L + 1) = softmax([x_i . u(i), w . (softmax(mask(x . uh)) . x) + b])  - Models/Layers.py:352-432 in one launch per
    direction (csrc/sdnet_scorer.hip).  u1 scores the slots i >= ES, u2 the first ES; all three (B, D)."""

    @staticmethod
    def forward(ctx, x, u1, u2, uh, w, b, mask, ES, mask_flag):
        lib = hip.kernels()
        for t in (x, u1, u2, uh, w, b):
            hip.require_gpu(t, torch.float32)
        nan_flag.ensure(x.device)
        B, L, D = x.shape
        probs = torch.empty(B, L + 1, dtype=torch.float32, device=x.device)
        a = torch.empty(B, L, dtype=torch.float32, device=x.device)
        lib.ruart_scorer_fwd(x, u1, u2, uh, w, b, mask, probs, a, B, L, D, int(ES), int(bool(mask_flag)), hip.stream_ptr())
        ctx.save_for_backward(x, u1, u2, uh, w, probs, a)
        ctx.ES = int(ES)
        return probs

    @staticmethod
    def backward(ctx, gp):
        lib = hip.kernels()
        x, u1, u2, uh, w, probs, a = ctx.saved_tensors
        B, L, D = x.shape
        gp = gp.contiguous()
        gx = torch.empty_like(x)
        gu1, gu2, guh, gwp = (torch.empty(B, D, dtype=torch.float32, device=x.device) for _ in range(4))
        gbp = torch.empty(B, dtype=torch.float32, device=x.device)
        lib.ruart_scorer_bwd(x, u1, u2, uh, w, probs, a, gp, gx, gu1, gu2, guh, gwp, gbp, B, L, D, ctx.ES, hip.stream_ptr())
        return gx, gu1, gu2, guh, colsum(gwp).view_as(w), gbp.sum().view(1), None, None, None


def fused_scorer(x, u1, u2, uh, w, b, mask, ES, mask_flag):
    """x (B, L, D), u1 / u2 / uh (B, D), w (D,) or (1, D), b (1,), mask (B, L): see _FusedScorer.  D % 4 == 0, L <= 1024."""
    return _FusedScorer.apply(x.contiguous(), u1.contiguous(), u2.contiguous(), uh.contiguous(), w.contiguous().view(-1), b.contiguous().view(1),
                              mask.to(torch.uint8).contiguous(), ES, mask_flag)


class _FusedScorerHeads(torch.autograd.Function):
    """probs (B, H + L) = softmax([s_0 .. s_{n_front-1}, x_i . u(i) ..., s_{n_front} .. s_{H-1}]) with H pooled heads
    s_h = w_h . (softmax(mask(x . uh_h)) . x) + b_h - Models/Layers.py:352-432 with ``yesno`` in one launch per direction
    (ruart_scorer_heads_fwd / _bwd, csrc/sdnet_scorer.hip).  u1 (B, D) scores the slots i >= ES, u2 the first ES (None with ES == 0)."""

    @staticmethod
    def forward(ctx, x, u1, u2, uh, w, b, mask, ES, n_front, mask_flag):
        lib = hip.kernels()
        for t in (x, u1, uh, w, b) + (() if u2 is None else (u2,)):
            hip.require_gpu(t, torch.float32)
        nan_flag.ensure(x.device)
        B, L, D = x.shape
        H = uh.shape[1]
        probs = torch.empty(B, H + L, dtype=torch.float32, device=x.device)
        a = torch.empty(B, H, L, dtype=torch.float32, device=x.device)
        lib.ruart_scorer_heads_fwd(x, u1, u1 if u2 is None else u2, uh, w, b, mask, probs, a, B, L, D, int(ES), H, int(n_front),
                                   int(bool(mask_flag)), hip.stream_ptr())
        ctx.save_for_backward(x, u1, u2, uh, w, probs, a)
        ctx.ES, ctx.n_front = int(ES), int(n_front)
        return probs

    @staticmethod
    def backward(ctx, gp):
        lib = hip.kernels()
        x, u1, u2, uh, w, probs, a = ctx.saved_tensors
        B, L, D = x.shape
        H = uh.shape[1]
        gp = gp.contiguous()
        gx = torch.empty_like(x)
        gu1, gu2 = (torch.empty(B, D, dtype=torch.float32, device=x.device) for _ in range(2))
        guh, gwp = (torch.empty(B, H, D, dtype=torch.float32, device=x.device) for _ in range(2))
        gbp = torch.empty(B, H, dtype=torch.float32, device=x.device)
        lib.ruart_scorer_heads_bwd(x, u1, u1 if u2 is None else u2, uh, w, probs, a, gp, gx, gu1, gu2, guh, gwp, gbp, B, L, D, ctx.ES, H,
                                   ctx.n_front, hip.stream_ptr())
        return gx, gu1, (None if u2 is None else gu2), guh, colsum(gwp.view(B, H * D)).view_as(w), gbp.sum(0), None, None, None, None


def fused_scorer_heads(x, u1, u2, uh, w, b, mask, ES, n_front, mask_flag):
    """x (B, L, D), u1 / u2 (B, D) (u2 None with ES == 0), uh (B, H, D), w (H, D), b (H,), mask (B, L): see _FusedScorerHeads and the
    argument contract in include/ruart_hip.h; a shape outside it raises ``hip.HipError`` with ``code`` hipErrorInvalidValue (1)."""
    return _FusedScorerHeads.apply(x.contiguous(), u1.contiguous(), None if u2 is None else u2.contiguous(), uh.contiguous(), w.contiguous(),
                                   b.contiguous(), mask.to(torch.uint8).contiguous(), ES, n_front, mask_flag)


# ---------------------------------------------------------------------------------------------------------
class _WholeLayerNorm(torch.autograd.Function):
    """F.layer_norm(x, x.size()) - normalisation over the WHOLE tensor, no affine (Models/Layers.py:167-168)."""

    @staticmethod
    def forward(ctx, x, eps):
        lib = hip.kernels()
        hip.require_gpu(x, torch.float32)
        nan_flag.ensure(x.device)
        y = torch.empty_like(x)
        stats = torch.empty(2, dtype=torch.float32, device=x.device)
        ws = _scratch(x.device, 2048)
        lib.ruart_whole_ln_fwd(x, y, stats, ws, x.numel(), eps, hip.stream_ptr())
        ctx.save_for_backward(y, stats)
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = hip.kernels()
        y, stats = ctx.saved_tensors
        gy = gy.contiguous()
        gx = torch.empty_like(y)
        ws = _scratch(y.device, 2048)
        lib.ruart_whole_ln_bwd(y, gy, stats, gx, ws, y.numel(), hip.stream_ptr())
        return gx, None


def _exchange_partials(group, width, fill, device):
    """Gather every rank's ``width`` per-block partials of ``group``: each rank writes its own slot of a zeroed (W, width) buffer
    (``fill(slot)``) and one all_reduce(SUM) adds zeros to everything else - an exact gather, on RCCL and gloo alike.  Returns the
    (W * width) buffer, rank-major, and W."""
    import torch.distributed as dist
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    buf = torch.zeros(world * width, dtype=torch.float32, device=device)
    fill(buf[rank * width:(rank + 1) * width])
    dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
    return buf, world


def whole_ln_global_fwd(x, eps, group):
    """Forward of the cross-rank whole-tensor layer norm: (y, stats) with stats = (mean, rstd) of the tensors of all ranks of
    ``group`` taken together.  Two exchanges of P = ruart_whole_ln_blocks() floats per rank.  Every rank's ``x`` has the same
    number of elements (VQA_Sampler deals W equal shards), so the global count is W * x.numel(), exact."""
    lib = hip.kernels()
    hip.require_gpu(x, torch.float32)
    nan_flag.ensure(x.device)
    P, n, st = lib.ruart_whole_ln_blocks(), x.numel(), hip.stream_ptr()
    part, world = _exchange_partials(group, P, lambda s: lib.ruart_whole_ln_partials(x, None, s, n, st), x.device)
    part2, _ = _exchange_partials(group, P, lambda s: lib.ruart_whole_ln_var_global(x, n, part, world, world * n, s, st), x.device)
    y = torch.empty_like(x)
    stats = torch.empty(2, dtype=torch.float32, device=x.device)
    lib.ruart_whole_ln_apply_global(x, y, n, eps, part, part2, world, world * n, stats, st)
    return y, stats


def whole_ln_global_bwd(y, gy, stats, group):
    """grad_x of the cross-rank whole-tensor layer norm: one exchange of 2 P floats per rank (sum gy, sum gy * y)."""
    lib = hip.kernels()
    gy = gy.contiguous()
    P, n, st = lib.ruart_whole_ln_blocks(), y.numel(), hip.stream_ptr()
    part, world = _exchange_partials(group, 2 * P, lambda s: lib.ruart_whole_ln_partials(gy, y, s, n, st), y.device)
    gx = torch.empty_like(y)
    lib.ruart_whole_ln_bwd_global(y, gy, stats, gx, n, part, world, world * n, st)
    return gx


class _GlobalWholeLayerNorm(torch.autograd.Function):
    """_WholeLayerNorm over the tensors of every rank of a process group taken together (opt['dp_global_batch'], DESIGN.md section
    6): the statistics of the global batch.  Forward and backward are collective calls on ``group``."""

    @staticmethod
    def forward(ctx, x, eps, group):
        y, stats = whole_ln_global_fwd(x, eps, group)
        ctx.group = group
        ctx.save_for_backward(y, stats)
        return y

    @staticmethod
    def backward(ctx, gy):
        y, stats = ctx.saved_tensors
        return whole_ln_global_bwd(y, gy, stats, ctx.group), None, None


def whole_layer_norm(x, eps=1e-5, group=None):
    """F.layer_norm(x, x.size()).  ``group`` (a torch.distributed process group): normalise over the tensors of all its ranks as if
    they were one, concatenated along the batch - every rank must call it, in the same order, with a tensor of the same size."""
    if group is None:
        return _WholeLayerNorm.apply(x.contiguous(), eps)
    return _GlobalWholeLayerNorm.apply(x.contiguous(), eps, group)


# ---------------------------------------------------------------------------------------------------------
# Dense projections of the trunk.  "x3": fp32 operands split into bf16 hi + lo inside the kernel, three 16-bit MFMA products
# (ruart_gemm_x3, relative error ~2^-16 per product, ~5x the fp32-MFMA rate); "fp32": torch.mm / addmm (rocBLAS, exact fp32
# MFMA) - the validation mode (SDNet runs in it when opt['bert_precision'] == 'fp32') and the fallback for tiny products.
@dataclasses.dataclass(frozen=True)
class TrunkMode:
    """How the trunk's ops compute.  One mode is in effect at a time (``trunk_mode()``); ``use_trunk_mode`` changes it for a scope.
    Every autograd Function copies what its backward needs into ``ctx`` during forward: a backward never reads the mode in effect."""
    gemm: str = "x3"                # forward products: "x3" | "fp32"
    # BACKWARD products (dX = dY W, dW = dY^T X, dW_hh) of an "x3" forward: "x3" (three bf16 products, fp32-class) or "x1" (one bf16
    # product with fp32 accumulation - what mixed-precision training uses for gradients); opt['ruart_trunk_grad_gemm']
    grad_gemm: str = "x3"
    defer_dw: bool = False          # weight gradients of _Linear in grouped launches at the end of backward (_flush_weight_grads)
    # variational-dropout masks of the projections' inputs read inside the GEMM's operand loads (see _Linear)
    fuse_masks: bool = os.environ.get("RUART_FUSE_MASK", "1") != "0"
    # GetFinalScores on the fused kernel (csrc/sdnet_scorer.hip); False: the op-by-op form (A/B runs, tests)
    fused_scorer: bool = os.environ.get("RUART_FUSED_SCORER", "1") != "0"

    _VALUES = {"gemm": ("x3", "fp32"), "grad_gemm": ("x3", "x1")}       # (no annotation: not a field)

    def __post_init__(self):
        for f in dataclasses.fields(self):
            v = getattr(self, f.name)
            if not (v in self._VALUES[f.name] if f.name in self._VALUES else isinstance(v, bool)):
                raise ValueError("TrunkMode.%s = %r: %s" % (f.name, v, " | ".join(map(repr, self._VALUES.get(f.name, (True, False))))))

    @property
    def backward_gemm(self):
        """form of the backward products of a Function whose forward ran in this mode"""
        return self.grad_gemm if self.gemm == "x3" else self.gemm

    def replace(self, **changes):
        unknown = sorted(set(changes) - {f.name for f in dataclasses.fields(self)})
        if unknown:
            raise ValueError("TrunkMode has no field %s" % ", ".join(unknown))
        return dataclasses.replace(self, **changes)


_mode = TrunkMode()         # module-level, not thread-local: autograd's backward threads must see the same default


def trunk_mode():
    """The TrunkMode in effect."""
    return _mode


@contextlib.contextmanager
def use_trunk_mode(mode=None, **changes):
    """Put ``mode`` - or the mode in effect with ``changes`` applied - into effect for the ``with`` body; the previous mode is back
    afterwards, on exceptions too.  Scopes nest; they must not overlap across threads (the store is one variable)."""
    global _mode
    saved = _mode
    _mode = (saved if mode is None else mode).replace(**changes)
    try:
        yield _mode
    finally:
        _mode = saved


_RETIRED = frozenset(("trunk_gemm", "trunk_grad_gemm", "defer_weight_grads", "fuse_operand_masks", "fused_scorer_enabled"))


def retired_name_error(module, name):
    """The AttributeError for ``module.name``: the mode used to be these five variables of this module and of layers."""
    if name in _RETIRED:
        return AttributeError("%s.%s is retired: read ops.trunk_mode(), change it with ops.use_trunk_mode()" % (module, name))
    return AttributeError("module %r has no attribute %r" % (module, name))


class RefusesRetiredNames(type(sys)):
    """Module type of ops and layers: assigning a retired name raises instead of creating an attribute that nothing reads.  (Reads
    of one are answered by the modules' ``__getattr__``, which only a missing name reaches.)"""

    def __setattr__(self, name, value):
        if name in _RETIRED:
            raise retired_name_error(self.__name__, name)
        super().__setattr__(name, value)


def __getattr__(name):
    raise retired_name_error(__name__, name)


sys.modules[__name__].__class__ = RefusesRetiredNames


def _one_unit_stride(t):
    """A 2-D view whose memory is row- or column-contiguous (what ruart_gemm_x3 addresses); copies only when it is neither."""
    r, c = t.shape
    if t.stride(1) == 1 and (t.stride(0) >= c or r == 1):
        return t
    if t.stride(0) == 1 and (t.stride(1) >= r or c == 1):
        return t
    return t.contiguous()


_X3_SPAN_LIMIT = 1 << 30


def _span(t):
    """elements between the first and the last element of a 2-D view, inclusive"""
    return (t.shape[0] - 1) * abs(t.stride(0)) + (t.shape[1] - 1) * abs(t.stride(1)) + 1 if t.numel() else 0


def mm(a, b, bias=None, mode=None, out=None, a_keep=None, b_keep=None, keep_scale=1.0, c_scale=None, rpm=1, residual=None):
    """a (M,K) . b (K,N) (+ bias (N,)) (+ residual (M,N)) -> (M,N) fp32 on the split-bf16 MFMA kernel - every size, down to a
    single row: no product of a step goes to the vendor library (see the module docstring).
    ``mode``: 'x3' | 'x1' | 'fp32' (torch.mm: the validation mode); default = ``trunk_mode().gemm`` (autograd Functions
    pass the mode of their forward).  ``out``: optional contiguous (M, N) destination.
    Variational-dropout masks fused into the product (each mask row is shared by ``rpm`` consecutive rows): ``a_keep`` (M/rpm, K) /
    ``b_keep`` (K/rpm, N) uint8 - the operand element is multiplied by ``keep_scale`` where the byte is non-zero and dropped where
    it is zero, inside the operand loads (one of the two per call, operand in its natural orientation); ``c_scale`` (M/rpm, N) fp32
    multiplies the output in the epilogue."""
    M, K = a.shape
    N = b.shape[1]
    mode = mode or trunk_mode().gemm
    if mode in ("x3", "x1"):           # the product modes have no CPU path (torch.mm below is the fp32 VALIDATION mode only)
        for t in (a, b):
            if not (t.is_cuda and t.dtype == torch.float32):
                raise hip.HipError("ops.mm: fp32 device tensors only (there is no CPU path); got %s on %s" % (t.dtype, t.device))
    use_x3 = mode in ("x3", "x1")

    def apply_keep(t, keep):
        return t * (keep.repeat_interleave(rpm, 0) != 0).to(t.dtype) * keep_scale

    if use_x3:
        a, b = _one_unit_stride(a), _one_unit_stride(b)
        # the kernels address an operand as base + 32-bit element offset (< 2^30 elements from the first to the last one, include/ruart_hip.h):
        # a view with a huge pitch is compacted here; an operand that is itself that large is split over its rows
        if _span(a) >= _X3_SPAN_LIMIT and a.numel() < _X3_SPAN_LIMIT:
            a = a.contiguous()
        if _span(b) >= _X3_SPAN_LIMIT and b.numel() < _X3_SPAN_LIMIT:
            b = b.contiguous()
        if _span(a) >= _X3_SPAN_LIMIT and a_keep is None and c_scale is None and M > 1:
            # (rows of the product are independent: a b-side mask applies to both halves unchanged - it masks b's K x N elements)
            out = torch.empty(M, N, dtype=torch.float32, device=a.device) if out is None else out
            h = M // 2
            mm(a[:h], b, bias, mode, out[:h], residual=None if residual is None else residual[:h], b_keep=b_keep, keep_scale=keep_scale, rpm=rpm)
            mm(a[h:], b, bias, mode, out[h:], residual=None if residual is None else residual[h:], b_keep=b_keep, keep_scale=keep_scale, rpm=rpm)
            return out
        if max(_span(a), _span(b)) >= _X3_SPAN_LIMIT:
            raise ValueError("ops.mm: an operand spans >= 2^30 elements in a layout the split-bf16 kernel cannot address; split the product")
        # the fused operand masks follow the operand's natural orientation only (and one operand at a time): otherwise multiply first
        if a_keep is not None and (a.stride(1) != 1 or b_keep is not None or max(M, K) >= (1 << 20)):
            a, a_keep = _one_unit_stride(apply_keep(a, a_keep)), None
        # (b with a unit row stride as well - a single column, or K == 1 over one column - is passed as K-contiguous below, a layout
        # the b_keep forms do not take: the entry point refuses it)
        if b_keep is not None and (b.stride(1) != 1 or b.stride(0) == 1 or max(N, K) >= (1 << 20)):
            b, b_keep = _one_unit_stride(apply_keep(b, b_keep)), None
    if not use_x3:
        if a_keep is not None:
            a = apply_keep(a, a_keep)
        if b_keep is not None:
            b = apply_keep(b, b_keep)
        r = torch.mm(a, b) if bias is None else torch.addmm(bias, a, b)
        if c_scale is not None:
            r = r * c_scale.repeat_interleave(rpm, 0)
        if residual is not None:
            r = r + residual
        return r if out is None else out.copy_(r)
    lib = hip.kernels()
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    elif not (out.is_contiguous() and out.shape == (M, N) and out.dtype == torch.float32):
        raise ValueError("mm(out=): a contiguous fp32 (M, N) tensor is required")
    sam, sak = (a.stride(0), 1) if a.stride(1) == 1 else (1, a.stride(1))
    sbk, sbn = (1, b.stride(1)) if b.stride(0) == 1 and b.stride(1) != 1 else (b.stride(0), 1)
    if b.stride(0) == 1 and b.stride(1) == 1:            # K == 1 or N == 1: either description is valid
        sbk, sbn = b.stride(0), 1
    for sc, shape, dt in ((a_keep, (M // rpm, K), torch.uint8), (b_keep, (K // rpm, N), torch.uint8), (c_scale, (M // rpm, N), torch.float32)):
        if sc is not None and not (sc.is_contiguous() and tuple(sc.shape) == shape and sc.dtype == dt):
            raise ValueError("mm: a fused mask must be a contiguous %s %s tensor" % (dt, shape))
    pkey = (M, N, K, sak == 1, sbk == 1)
    ws_bytes = _PLAN_BYTES.get(pkey)
    if ws_bytes is None:                                   # (the plan is a pure function of the shape and the two layouts: asked once)
        nbytes = ctypes.c_size_t(0)
        lib.ruart_gemm_x3_plan(M, N, K, int(sak == 1), int(sbk == 1), None, ctypes.byref(nbytes))
        ws_bytes = _PLAN_BYTES[pkey] = int(nbytes.value)
    ws = _scratch(a.device, ws_bytes // 4, "x3") if ws_bytes else None
    fn = lib.ruart_gemm_x1 if mode == "x1" else lib.ruart_gemm_x3
    ldr = 0
    if residual is not None:
        if not (residual.shape == (M, N) and residual.dtype == torch.float32 and residual.stride(1) == 1):
            residual = residual.contiguous()
        ldr = residual.stride(0)
    fn(a, sam, sak, b, sbk, sbn, bias, residual, ldr, hip.ACT_NONE, out, N, M, N, K, ws, ws_bytes, a_keep, b_keep, float(keep_scale),
       c_scale, int(rpm), hip.stream_ptr())
    return out


def colsum(x):
    """x.sum(0) of a 2-D fp32 device matrix in two ordered stages (ruart_colsum_f32): the bias gradients of the trunk's projections -
    torch's generic reduction takes 33 us for a (6400, 1000) gradient, this 8."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[0] > 64):
        return x.sum(0)
    rows, cols = x.shape
    lib = hip.kernels()
    out = torch.empty(cols, dtype=torch.float32, device=x.device)
    ws = _scratch(x.device, int(lib.ruart_colsum_f32_ws_floats(rows, cols)), "colsum")
    lib.ruart_colsum_f32(x, x.stride(0), rows, cols, out, 0, ws, hip.stream_ptr(x.device))
    return out


# ---- deferred weight gradients ------------------------------------------------------------------------------------------------
# A training step has ~45 nn.Linear sites in the trunk.  Alone, each dW = dY^T X is a small output with a long reduction: 10-30 % of
# the chip for 20-50 us plus a split-K reduction launch.  With ``defer_dw`` on in the mode of its forward (opt['ruart_defer_dw']), the
# backward of ``_Linear`` only RECORDS (dY, X, W) and queues one end-of-backward callback with the autograd engine; the callback runs
# all recorded products as ruart_gemm_x3_tn_grouped launches (one per alignment class and wave), writes / accumulates ``W.grad`` and
# fires the parameters' post-accumulate hooks (dp.GradSync) - all still inside ``loss.backward()``, so callers see nothing new.
# Every product is tiled, split and summed exactly as the single launch would: bitwise the same gradients.
_deferred = []


def _flush_weight_grads():
    global _deferred
    items, _deferred = _deferred, []
    if not items:
        return
    lib = hip.kernels()
    dev = items[0][0].device
    with torch.cuda.device(dev):
        # the operands were produced on the trunk's three streams: this (the caller's) stream waits for each of them once, and the
        # caching allocator learns that their memory is read here
        cur = torch.cuda.current_stream(dev)
        for st in {it[3] for it in items}:
            if st != cur:
                cur.wait_stream(st)
        for gy, xm, _, st in items:
            if st != cur:
                gy.record_stream(cur)
                xm.record_stream(cur)
        # waves: a weight's k-th contribution goes to wave k (problems of one call must write distinct outputs)
        seen, waves = {}, []
        for gy, xm, w, _ in items:
            k = seen.get(id(w), 0)
            seen[id(w)] = k + 1
            while len(waves) <= k:
                waves.append([])
            waves[k].append((gy, xm, w))
        out = {}
        for k, wave in enumerate(waves):
            arr = (hip.X3TnProblemC * len(wave))()
            for i, (gy, xm, w) in enumerate(wave):
                if k == 0:
                    out[id(w)] = (w, torch.empty(w.shape, dtype=torch.float32, device=dev))
                c = out[id(w)][1]
                q = arr[i]
                q.A, q.B, q.C = gy.data_ptr(), xm.data_ptr(), c.data_ptr()
                q.lda, q.ldb, q.ldc = gy.stride(0), xm.stride(0), c.stride(0)
                q.M, q.N, q.K = gy.shape[1], xm.shape[1], gy.shape[0]
                q.accumulate = 1 if k > 0 else 0
            nbytes = int(lib.ruart_gemm_x3_tn_grouped_ws(arr, len(wave)))
            ws = _scratch(dev, nbytes // 4, "x3g") if nbytes else None
            lib.ruart_gemm_x3_tn_grouped(arr, len(wave), ws, nbytes, hip.stream_ptr(dev))
        for w, g in out.values():
            if w.grad is None:
                w.grad = g
            else:
                w.grad = w.grad + g
            for hook in (getattr(w, "_post_accumulate_grad_hooks", None) or {}).values():
                hook(w)


def _defer_weight_grad(gy, xm, w):
    """Record dW += gy^T xm for the end of this backward pass; False when the operands do not fit the grouped kernel."""
    if not (gy.dim() == 2 and xm.dim() == 2 and gy.stride(1) == 1 and xm.stride(1) == 1 and w.is_leaf and w.dim() == 2
            and w.shape == (gy.shape[1], xm.shape[1]) and gy.dtype == torch.float32 and xm.dtype == torch.float32):
        return False
    if torch.cuda.is_current_stream_capturing():
        return False
    if not _deferred:
        torch.autograd.Variable._execution_engine.queue_callback(_flush_weight_grads)
    _deferred.append((gy, xm, w, torch.cuda.current_stream(gy.device)))
    return True


class _Linear(torch.autograd.Function):
    """y = (x * mask) W^T (+ b) with x (rows, K), W (N, K), mask (rows / rpm, K) or None, on ruart_gemm_x3.
    With the mask's one-byte-per-element form at hand (``keep``, ``keep_scale``: layers.MaskBank) no pass of its own applies it: the
    forward reads the bytes beside x in the operand loads (a_keep), dW = dY^T (x * mask) reads them beside x again (b_keep), and
    dX = (dY W) * mask comes out of the GEMM epilogue (c_scale) - x * mask is never materialised.  Without it (a mask drawn outside the
    bank; ``fuse_masks`` off / RUART_FUSE_MASK=0: the form of rounds 2-3) the forward multiplies once and keeps the product."""

    @staticmethod
    def forward(ctx, x, w, b, mask, rpm, wparts=None, keep=None, keep_scale=1.0):
        """``wparts``: [(Parameter, row0, row1), ...] when ``w`` is a concatenation of parameters along its rows (the two directions of a
        BiLSTM input projection): deferred weight gradients are then taken per part, straight into the parameters."""
        m = trunk_mode()
        ctx.mode, ctx.defer_dw = m.backward_gemm, m.defer_dw       # the backward's product form and deferral are the forward's
        fused = (mask is not None and keep is not None and m.fuse_masks and m.gemm == "x3" and not m.defer_dw
                 and x.stride(1) == 1 and x.shape[0] < (1 << 20) and x.shape[1] < (1 << 20))
        ctx.fused, ctx.keep_scale = fused, float(keep_scale)
        xm = x if (mask is None or fused) else (x.view(-1, rpm, x.shape[1]) * mask.unsqueeze(1)).view(x.shape)
        ctx.save_for_backward(xm, w, mask, keep if fused else None)
        # the Parameter behind w, when w IS one (a grouped end-of-backward product writes its .grad directly, see above)
        ctx.wparam = w if (isinstance(w, torch.nn.Parameter) and w.requires_grad) else None
        ctx.wparts = wparts
        ctx.has_bias = b is not None
        ctx.rpm = rpm
        return mm(xm, w.t(), b, a_keep=keep if fused else None, keep_scale=keep_scale, rpm=rpm)

    @staticmethod
    def backward(ctx, gy):
        xm, w, mask, keep = ctx.saved_tensors
        gx = mm(gy, w, mode=ctx.mode, c_scale=mask, rpm=ctx.rpm) if ctx.needs_input_grad[0] else None
        gw = None
        if ctx.needs_input_grad[1]:
            wp, parts = ctx.wparam, ctx.wparts
            done = False
            if ctx.defer_dw and ctx.mode == "x3" and gy.stride(1) == 1 and not ctx.fused:
                if wp is not None:
                    done = _defer_weight_grad(gy, xm, wp)
                elif parts and all(p.requires_grad and p.is_leaf for p, _, _ in parts):
                    done = all([_defer_weight_grad(gy[:, r0:r1], xm, p) for p, r0, r1 in parts])
            if not done:
                gw = mm(gy.t(), xm, mode=ctx.mode, b_keep=keep, keep_scale=ctx.keep_scale, rpm=ctx.rpm)
        gb = colsum(gy) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        return gx, gw, gb, None, None, None, None, None


class _AddMM(torch.autograd.Function):
    """base + x W^T in one launch (the residual rides in the GEMM epilogue): the recurrent product of a Python-stepped LSTM
    step (`multi2one`) added to the step's input projection (Models/SDNet.py:269-271 via nn.LSTM)."""

    @staticmethod
    def forward(ctx, base, x, w):
        ctx.save_for_backward(x, w)
        ctx.mode = trunk_mode().backward_gemm
        return mm(x, w.t(), residual=base)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = gy.contiguous()
        gx = mm(gy, w, mode=ctx.mode) if ctx.needs_input_grad[1] else None
        gw = mm(gy.t(), x, mode=ctx.mode) if ctx.needs_input_grad[2] else None
        return (gy if ctx.needs_input_grad[0] else None), gx, gw


class _MatMul2D(torch.autograd.Function):
    """a (M, K) . b (K, N) for two fp32 device matrices, both differentiable, every product on ruart_gemm_x3."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        ctx.mode = trunk_mode().backward_gemm
        return mm(a, b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous()
        ga = mm(g, b.t(), mode=ctx.mode) if ctx.needs_input_grad[0] else None
        gb = mm(a.t(), g, mode=ctx.mode) if ctx.needs_input_grad[1] else None
        return ga, gb


def matmul2d(a, b):
    return _MatMul2D.apply(a, b)


def addmm(base, x, w):
    """base (M, N) + x (M, K) . w (N, K)^T."""
    if trunk_mode().gemm != "x3":             # exact-fp32 validation mode
        return torch.addmm(base, x, w.t())
    if not x.is_cuda:
        raise hip.HipError("ops.addmm: device tensors only (there is no CPU path)")
    return _AddMM.apply(base, x.contiguous(), w)


def linear(x, w, b=None, mask=None, wparts=None):
    """F.linear for fp32 device tensors of any leading shape, through ``mm``.  ``mask`` (B, K) with x (B, T, K): variational
    dropout (x * mask[:, None, :]) applied inside the op.  A mask that carries its byte form (``mask.keep`` uint8 (B, K), ``mask.keep_scale``
    = 1/(1-p): what layers.MaskBank hands out) is read inside the three products; any other mask costs one multiply in the forward."""
    if trunk_mode().gemm != "x3":             # exact-fp32 validation mode
        if mask is not None:
            x = x * mask.unsqueeze(1)
        return torch.nn.functional.linear(x, w, b)
    if not x.is_cuda:
        raise hip.HipError("ops.linear: device tensors only (there is no CPU path)")
    lead = x.shape[:-1]
    rpm = 1
    keep, keep_scale = None, 1.0
    if mask is not None:
        if x.dim() != 3 or mask.shape != (x.shape[0], x.shape[2]):
            raise ValueError("linear(mask=): x (B, T, K) with mask (B, K)")
        rpm = x.shape[1]
        keep, keep_scale = getattr(mask, "keep", None), getattr(mask, "keep_scale", 1.0)      # layers.MaskBank attaches them
        mask = mask.contiguous()
    x2 = x.reshape(-1, x.shape[-1])
    y = _Linear.apply(x2, w, b, mask, rpm, wparts, keep, keep_scale)
    return y.view(*lead, w.shape[0])


# ---------------------------------------------------------------------------------------------------------
def _padded16(x, dtype, mult=256):
    """fp32 (M, K) -> 16-bit (ceil(M / mult) * mult, K), zero rows at the end (the MFMA GEMM's row granularity)."""
    M, K = x.shape
    Mp = (M + mult - 1) // mult * mult
    y = torch.empty(Mp, K, dtype=dtype, device=x.device)
    y[:M].copy_(x)
    if Mp > M:
        y[M:].zero_()
    return y


def _gemm16(a16, w16, bias, M_out, dt):
    """a16 (Mp, K) . w16 (N, K)^T (+ bias) -> fp32 (M_out, N) on ruart_gemm_16_nt (the encoder's 256x256 MFMA kernel)."""
    lib = hip.kernels()
    Mp, K = a16.shape
    N = w16.shape[0]
    out = torch.empty(Mp, N, dtype=torch.float32, device=a16.device)
    lib.ruart_gemm_16_nt(a16, K, w16, K, bias, None, 0, dt, out, N, hip.DT_F32, Mp, N, K, hip.ACT_NONE, dt, hip.stream_ptr())
    return out[:M_out]


class _Linear16(torch.autograd.Function):
    """y = x W^T + b for fp32 x (M, K), W (N, K) with 16-bit MFMA operands (N, K multiples of 256 / 128): forward in f16 (11
    significand bits; activations are O(1)-O(100)), dX = dY W in bf16 (gradients need the exponent range), both on the encoder's
    GEMM kernel with on-the-fly casts; dW = dY^T X stays on the split-bf16 kernel (its reduction runs over all M rows)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        return _gemm16(_padded16(x, torch.float16), w.to(torch.float16), b, x.shape[0], hip.DT_F16)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = gy.contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = _gemm16(_padded16(gy, torch.bfloat16), w.t().contiguous().to(torch.bfloat16), None, gy.shape[0], hip.DT_BF16)
        if ctx.needs_input_grad[1]:
            gw = _dw_bf16(gy, x)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = gy.sum(0)
        return gx, gw, gb


def _dw_bf16(gy, x):
    """dW (N, K) = gy^T . x for gy (rows, N), x (rows, K) fp32: one bf16 MFMA product with fp32 accumulation
    (ruart_gemm_bf16_tn), or the split-bf16 kernel when the operands are not laid out for it."""
    rows, N = gy.shape
    K = x.shape[1]
    if not (gy.is_contiguous() and x.is_contiguous() and N % 4 == 0 and K % 4 == 0 and gy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0):
        return mm(gy.t(), x, mode="x3")
    nbytes = ctypes.c_size_t(0)
    hip.kernels().ruart_gemm_x3_plan(N, K, rows, 0, 0, None, ctypes.byref(nbytes))
    ws = _scratch(gy.device, nbytes.value // 4, "x3") if nbytes.value else None
    out = torch.empty(N, K, dtype=torch.float32, device=gy.device)
    # the raw handle: a non-zero code here means "not a shape of this kernel" and selects the split-bf16 product, it is not an error
    rc = hip.load().ruart_gemm_bf16_tn(gy, N, x, K, out, K, N, K, rows, ws, nbytes.value, hip.stream_ptr())
    if rc != 0:
        return mm(gy.t(), x, mode="x3")
    return out


def linear16(x, w, b=None):
    """``linear`` with 16-bit MFMA operands for the two row-parallel products (see _Linear16); falls back to ``linear`` for shapes
    the encoder's GEMM does not take."""
    N, K = w.shape
    if not x.is_cuda or x.dim() != 2 or N % 256 or K % 256:
        return linear(x, w, b)
    return _Linear16.apply(x.contiguous(), w, b)


# ---------------------------------------------------------------------------------------------------------
LSTM_MAX_HIDDEN = 256           # up to here the recurrence is one persistent launch (ruart_lstm_fwd / _bwd); StackedBRNN routes by it

_lstm_ws_bytes = {}             # (h, ndir) -> ruart_lstm_ws_bytes


def _lstm_workspace(h, ndir, device):
    """Workspace of ONE ruart_lstm_fwd / _bwd call, or None where the library needs none (W_hh resident in registers).  An ordinary
    allocation per call, not ``_scratch``: the trunk's streams run LSTM layers concurrently, and a shared buffer would be rewritten
    under a running kernel."""
    n = _lstm_ws_bytes.get((h, ndir))
    if n is None:
        out = ctypes.c_size_t()
        hip.kernels().ruart_lstm_ws_bytes(h, ndir, ctypes.byref(out))
        n = _lstm_ws_bytes[(h, ndir)] = out.value
    return torch.empty(n, dtype=torch.uint8, device=device) if n else None


class _LstmRecurrence(torch.autograd.Function):
    """Sequential part of one (Bi)LSTM layer.  xproj (B,T,ndir*4h) already holds x W_ih^T + b_ih + b_hh.  The library chooses the
    kernels by the hidden size; layers above LSTM_MAX_HIDDEN are refused by it (HipError)."""

    @staticmethod
    def forward(ctx, xproj, w_hh, ndir):
        lib = hip.kernels()
        hip.require_gpu(xproj, torch.float32)
        hip.require_gpu(w_hh, torch.float32)
        nan_flag.ensure(xproj.device)
        B, T, G = xproj.shape
        h = G // (4 * ndir)
        y = torch.empty(B, T, ndir * h, dtype=torch.float32, device=xproj.device)
        need = xproj.requires_grad or w_hh.requires_grad
        gates = torch.empty_like(xproj) if need else None
        cells = torch.empty_like(y) if need else None
        hprev = torch.empty_like(y) if w_hh.requires_grad else None
        ws = _lstm_workspace(h, ndir, xproj.device)
        lib.ruart_lstm_fwd(xproj, w_hh, y, gates, cells, hprev, B, T, h, ndir, ws, ws.numel() if ws is not None else 0, hip.stream_ptr())
        ctx.ndir, ctx.h = ndir, h
        ctx.mode = trunk_mode().backward_gemm
        ctx.save_for_backward(w_hh, gates, cells, hprev)
        ctx.shape = y.shape
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = hip.kernels()
        w_hh, gates, cells, hprev = ctx.saved_tensors
        ndir, h = ctx.ndir, ctx.h
        B, T, _ = ctx.shape
        gy = gy.contiguous()
        gx = torch.empty_like(gates)
        ws = _lstm_workspace(h, ndir, gy.device)
        lib.ruart_lstm_bwd(gy, w_hh, gates, cells, gx, B, T, h, ndir, ws, ws.numel() if ws is not None else 0, hip.stream_ptr())
        # grad_W_hh[d] = sum_{b,t} da[b,t,d] (x) h_prev[b,t,d]: one GEMM per direction on column slices (strided views, no copies)
        gw = None
        if ctx.needs_input_grad[1]:
            gx2, hp2 = gx.view(B * T, -1), hprev.view(B * T, -1)
            if ndir == 1:
                gw = mm(gx2.t(), hp2, mode=ctx.mode).unsqueeze(0)
            else:
                # both directions in ONE product (ndir 4h x ndir h over the B T rows) whose diagonal blocks are the two gradients: the
                # off-diagonal half of the work is wasted, but each of these products is a 30 us launch-and-latency affair plus its
                # own split-K reduction - 22 of them per step before, 11 now
                full = mm(gx2.t(), hp2, mode=ctx.mode)
                gw = torch.stack([full[d * 4 * h:(d + 1) * 4 * h, d * h:(d + 1) * h] for d in range(ndir)], 0)
        return gx, gw, None


class _LstmPackParams(torch.autograd.Function):
    """(w_ih, w_ih_r, b_ih, b_hh, b_ih_r, b_hh_r, w_hh, w_hh_r) -> (w, b, whh) as lstm_layer's kernels take them
    (ruart_lstm_pack_params); the backward hands out slices of the incoming gradients - no launch."""

    @staticmethod
    def forward(ctx, w_ih, w_ih_r, b_ih, b_hh, b_ih_r, b_hh_r, w_hh, w_hh_r):
        G, K = w_ih.shape
        h = w_hh.shape[1]
        if not (w_ih_r.shape == (G, K) and w_hh.shape == w_hh_r.shape == (G, h)
                and b_ih.shape == b_hh.shape == b_ih_r.shape == b_hh_r.shape == (G,)):
            raise ValueError("lstm_layer: the two directions must have the same shapes")
        w = torch.empty(2 * G, K, dtype=torch.float32, device=w_ih.device)
        b = torch.empty(2 * G, dtype=torch.float32, device=w_ih.device)
        whh = torch.empty(2, G, h, dtype=torch.float32, device=w_ih.device)
        hip.kernels().ruart_lstm_pack_params(w_ih, w_ih_r, b_ih, b_hh, b_ih_r, b_hh_r, w_hh, w_hh_r, w, b, whh, G, K, h,
                                             hip.stream_ptr(w_ih.device))
        ctx.G = G
        return w, b, whh

    @staticmethod
    def backward(ctx, gw, gb, gwhh):
        G = ctx.G
        gw0 = gw1 = gb0 = gb1 = gh0 = gh1 = None
        if gw is not None:
            gw0, gw1 = gw[:G], gw[G:]
        if gb is not None:
            gb0, gb1 = gb[:G], gb[G:]
        if gwhh is not None:
            gh0, gh1 = gwhh[0], gwhh[1]
        return gw0, gw1, gb0, gb0, gb1, gb1, gh0, gh1


def lstm_layer(x, w_ih, w_hh, b_ih, b_hh, w_ih_r=None, w_hh_r=None, b_ih_r=None, b_hh_r=None, mask=None):
    """One nn.LSTM layer (batch_first, zero state), uni- or bidirectional, on the persistent HIP recurrence.
    Parameters use torch's nn.LSTM layout so checkpoints load unchanged."""
    bidir = w_ih_r is not None
    wparts = None
    if bidir:
        params = (w_ih, w_ih_r, b_ih, b_hh, b_ih_r, b_hh_r, w_hh, w_hh_r)
        if trunk_mode().gemm == "x3" and all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in params):
            w, b, whh = _LstmPackParams.apply(*params)          # one launch instead of two cats, two adds and a stack
        else:
            w = torch.cat([w_ih, w_ih_r], 0)
            b = torch.cat([b_ih + b_hh, b_ih_r + b_hh_r], 0)
            whh = torch.stack([w_hh, w_hh_r], 0)
        if isinstance(w_ih, torch.nn.Parameter) and isinstance(w_ih_r, torch.nn.Parameter):
            wparts = [(w_ih, 0, w_ih.shape[0]), (w_ih_r, w_ih.shape[0], w.shape[0])]
    else:
        w, b, whh = w_ih, b_ih + b_hh, w_hh.unsqueeze(0)
    xproj = linear(x, w, b, mask=mask, wparts=wparts)   # mask: the input's variational-dropout mask, fused into the projection
    return _LstmRecurrence.apply(xproj.contiguous(), whh.contiguous(), 2 if bidir else 1)


# ---------------------------------------------------------------------------------------------------------
class _LstmCell(torch.autograd.Function):
    """Pointwise part of one LSTM step over a ragged, length-sorted batch (see ruart_lstm_cell_fwd)."""

    @staticmethod
    def forward(ctx, pre, h_prev, c_prev, n_active):
        lib = hip.kernels()
        for t in (pre, h_prev, c_prev):
            hip.require_gpu(t, torch.float32)
        N, h = h_prev.shape
        h_out, c_out = torch.empty_like(h_prev), torch.empty_like(c_prev)
        acts = torch.empty_like(pre)
        lib.ruart_lstm_cell_fwd(pre, h_prev, c_prev, h_out, c_out, acts, n_active, N, h, hip.stream_ptr())
        ctx.save_for_backward(acts, c_prev, c_out)
        ctx.n_active = n_active
        return h_out, c_out

    @staticmethod
    def backward(ctx, gh, gc):
        lib = hip.kernels()
        acts, c_prev, c_out = ctx.saved_tensors
        N, h = c_prev.shape
        gh = gh.contiguous() if gh is not None else None
        gc = gc.contiguous() if gc is not None else None
        g_pre = torch.empty_like(acts)
        g_h, g_c = torch.empty_like(c_prev), torch.empty_like(c_prev)
        lib.ruart_lstm_cell_bwd(gh, gc, acts, c_prev, c_out, g_pre, g_h, g_c, ctx.n_active, N, h, hip.stream_ptr())
        return g_pre, g_h, g_c, None


def lstm_cell(pre, h_prev, c_prev, n_active):
    """pre (n_active, 4h), h_prev / c_prev (N, h) -> (h, c) of all N rows; rows >= n_active pass through."""
    return _LstmCell.apply(pre.contiguous(), h_prev.contiguous(), c_prev.contiguous(), int(n_active))


# ---------------------------------------------------------------------------------------------------------
class _RowScale(torch.autograd.Function):
    """y[w] = x[w] * mask[row_of[w]] for a packed (words, D) fp32 matrix and one mask row per item (ruart_rows_scale): the mask rows are
    read through the index inside the kernel, in the forward and in the backward - no (words, D) copy of the mask exists."""

    @staticmethod
    def forward(ctx, x, mask, row_of):
        y = torch.empty_like(x)
        hip.kernels().ruart_rows_scale(x, x.stride(0), mask, mask.stride(0), row_of, y, y.stride(0), x.shape[0], x.shape[1],
                                       hip.stream_ptr(x.device))
        ctx.save_for_backward(mask, row_of)
        return y

    @staticmethod
    def backward(ctx, g):
        mask, row_of = ctx.saved_tensors
        if g.stride(1) != 1 or g.stride(0) % 4 or g.data_ptr() % 16:
            g = g.contiguous()
        gx = torch.empty(g.shape, dtype=torch.float32, device=g.device)
        hip.kernels().ruart_rows_scale(g, g.stride(0), mask, mask.stride(0), row_of, gx, gx.stride(0), g.shape[0], g.shape[1],
                                       hip.stream_ptr(g.device))
        return gx, None, None


def rows_scale(x, mask, row_of):
    """x (W, D) * mask (N, D)[row_of (W,)] on the fused kernel when the layout allows it (fp32 device tensors, D % 4 == 0, aligned rows),
    else the gather-and-multiply of torch."""
    if (x.is_cuda and x.dtype == torch.float32 and mask.dtype == torch.float32 and x.dim() == 2 and x.shape[0] > 0 and x.shape[1] % 4 == 0
            and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 and mask.stride(1) == 1 and mask.stride(0) % 4 == 0
            and mask.data_ptr() % 16 == 0 and row_of.dtype == torch.int64 and row_of.is_contiguous()):
        return _RowScale.apply(x, mask, row_of)
    return x * mask[row_of]


# ---------------------------------------------------------------------------------------------------------
def embedding_grad(gy, sort, shape):
    """Gradient of an embedding table (``shape`` = (V, D)) from the (n, D) gradient rows of its lookups and the host-prepared sort of
    their ids (batch._sort_ids): 3 tensors = one workgroup per looked-up row; 4 tensors = the two-level form for rows with very many
    occurrences.  Ordered sums, no atomics: the same bits every run."""
    V, D = shape
    lib = hip.kernels()
    gw = torch.zeros(V, D, dtype=torch.float32, device=gy.device)
    gy = gy.reshape(-1, D).contiguous()
    if len(sort) == 3:
        order, seg_start, seg_row = sort
        lib.ruart_embedding_bwd_sorted(gy, order, seg_start, seg_row, seg_row.numel(), D, gw, hip.stream_ptr(gy.device))
    else:
        order, sub_start, row_first, row_id = sort
        n_sub = sub_start.numel() - 1
        ws = torch.empty(max(n_sub, 1), D, dtype=torch.float32, device=gy.device)
        lib.ruart_embedding_bwd_split(gy, order, sub_start, n_sub, row_first, row_id, row_id.numel(), D, ws, gw,
                                      hip.stream_ptr(gy.device))
    return gw


class _Embedding(torch.autograd.Function):
    """weight[ids] whose backward uses a host-prepared sort of the ids (``embedding_grad``) instead of sorting on the device: ``sort`` =
    int32 device tensors from batch.BatchIndex (padding_idx already left out)."""

    @staticmethod
    def forward(ctx, weight, ids, *sort):
        ctx.save_for_backward(*sort)
        ctx.wshape = weight.shape
        return weight.index_select(0, ids.reshape(-1)).view(*ids.shape, weight.shape[1])

    @staticmethod
    def backward(ctx, gy):
        return (embedding_grad(gy, ctx.saved_tensors, ctx.wshape), None) + (None,) * len(ctx.saved_tensors)


def embedding(module, ids, sort=None):
    """``module(ids)`` for an nn.Embedding; with ``sort`` (and a trainable fp32 table on the device) the gradient takes the
    host-sorted path."""
    w = module.weight
    if sort is None or not w.requires_grad or not torch.is_grad_enabled() or not w.is_cuda or w.dtype != torch.float32:
        return module(ids)
    return _Embedding.apply(w, ids, *sort)
