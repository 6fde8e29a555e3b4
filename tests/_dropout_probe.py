"""Dropout masks of the trainable encoder's kernels, recovered THROUGH the kernels (GPU test infrastructure): nothing here restates
the hash of csrc/common.h.  The masks depend on (seed, element index) only, so inputs are chosen that make every output entry a known
constant times its multiplier.  Every recovered entry must be 0 or, within f16 rounding, the constant / (1 - p); anything else fails."""
import numpy as np
import torch

from ruart_amd import hip

DEV = "cuda:0"
F16_ROUNDINGS = 2.0 ** -10          # two f16 roundings (2^-11 each) of one product: the probability and the output


def ln_mask(lib, R, H, p, seed, post):
    """(R, H) float64 multiplier of ruart_ln_train_fwd's dropout: 0 or 1 / (1 - p).  post = 0 (dense -> dropout -> + input ->
    LayerNorm): a constant input and no residual, the kept pre-LayerNorm entries are the constant / (1 - p).  post = 1 (the embeddings:
    LayerNorm -> dropout): gamma = 0, beta = 1 makes the LayerNorm output 1 everywhere, so y != 0 is the mask."""
    st = hip.stream_ptr()
    y = torch.empty(R, H, dtype=torch.float16, device=DEV)
    pre = torch.empty(R, H, dtype=torch.float16, device=DEV)
    stats = torch.empty(R, 2, dtype=torch.float32, device=DEV)
    if post:
        x = torch.randn(R, H, generator=torch.Generator().manual_seed(1)).to(DEV)
        gamma, beta, const, out = torch.zeros(H, device=DEV), torch.ones(H, device=DEV), 1.0, y
    else:
        x = torch.full((R, H), 2.0, device=DEV)
        gamma, beta, const, out = torch.ones(H, device=DEV), torch.zeros(H, device=DEV), 2.0, pre
    rc = lib.ruart_ln_train_fwd(hip.ptr(x), H, None, H, hip.ptr(gamma), hip.ptr(beta), 1e-12, float(p), int(seed), int(post), hip.ptr(y),
                                hip.ptr(pre), hip.ptr(stats), H, R, H, st)
    assert rc == 0
    raw = out.double().cpu() / const * (1.0 - p)                  # 0 or 1
    keep = raw != 0
    assert float((raw[keep] - 1.0).abs().max()) <= 2.0 ** -11, "a LayerNorm-site multiplier that is neither 0 nor 1 / (1 - p)"
    return keep.double() / (1.0 - p)


def attn_fwd(lib, qkv16, heads, win, ch, tok_lo, p, seed):
    """context rows (T, H) f16 of the window kernel (win = [q0, q1]) and the *_long kernel (ch = [q0, q1, k0, k1, ...]) on one stream"""
    T, H = qkv16.shape[0], heads * 64
    st = hip.stream_ptr()
    ctx = torch.zeros(T, H, dtype=torch.float16, device=DEV)
    nw, nc = int(win[0].numel()), int(ch[0].numel()) if ch is not None else 0
    if nw:
        assert lib.ruart_attn_train_fwd(hip.ptr(qkv16), 3 * H, hip.ptr(ctx), H, H, heads, nw, hip.ptr(win[0]), hip.ptr(win[1]), hip.ptr(tok_lo),
                                        float(p), int(seed), st) == 0
    if nc:
        lse = torch.empty(T, heads, device=DEV)
        assert lib.ruart_attn_train_fwd_long(hip.ptr(qkv16), 3 * H, hip.ptr(ctx), H, H, heads, nc, hip.ptr(ch[0]), hip.ptr(ch[1]), hip.ptr(ch[2]),
                                             hip.ptr(ch[3]), float(p), int(seed), hip.ptr(lse), st) == 0
    return ctx


def attn_masks(lib, heads, cu, win, ch, tok_lo, p, seed):
    """Per sequence the (heads, n, n) float64 multiplier of the attention-probability dropout: 0 or 1 / (1 - p).

    Q = 0 makes every in-sequence probability exactly 1 / n; one-hot V rows then copy the dropped probabilities into the context:
    window starting at q0:  V[t, h*64 + c] = 1 iff c == t - q0          ->  ctx[i, h, c] = Pd[i, key q0 + c]
    *_long, pass b:         V[t, h*64 + c] = 1 iff t - k0 == 64 b + c   ->  ctx[i, h, c] = Pd[i, key k0 + 64 b + c]   (all long
    sequences share a pass).  Keys of another sequence of the window, and columns past the sequence's end, must come out exactly 0.
    Returns (masks, worst relative deviation of a kept entry from 1 / (n (1 - p)))."""
    cu = np.asarray(cu, dtype=np.int64)
    T, H = int(cu[-1]), heads * 64
    wq0 = win[0].cpu().numpy().astype(np.int64) if win[0].numel() else np.zeros(0, np.int64)
    wq1 = win[1].cpu().numpy().astype(np.int64) if win[0].numel() else np.zeros(0, np.int64)
    n_ch = int(ch[0].numel()) if ch is not None else 0
    ck0 = ch[2].cpu().numpy().astype(np.int64) if n_ch else np.zeros(0, np.int64)
    lens = np.diff(cu)
    is_long = np.isin(cu[:-1], ck0)
    # every short sequence lies in exactly one window
    win_of = {}
    for s in np.nonzero(~is_long)[0]:
        w = np.nonzero((wq0 <= cu[s]) & (cu[s + 1] <= wq1))[0]
        assert len(w) == 1, "sequence %d is in no window" % s
        win_of[int(s)] = int(wq0[w[0]])
    n_pass = max(1, int(-(-lens[is_long].max() // 64))) if is_long.any() else 1
    raw = [torch.zeros(heads, int(n), int(n), dtype=torch.float64) for n in lens]
    for b in range(n_pass):
        V = torch.zeros(T, heads, 64)
        for s in range(len(lens)):
            t = np.arange(cu[s], cu[s + 1])
            c = t - cu[s] - 64 * b if is_long[s] else (t - win_of[s] if b == 0 else np.full_like(t, -1))
            ok = (c >= 0) & (c < 64)
            V[torch.from_numpy(t[ok]), :, torch.from_numpy(c[ok])] = 1.0
        qkv = torch.zeros(T, 3 * H, dtype=torch.float16)
        qkv[:, 2 * H:] = V.reshape(T, H).half()
        none = [torch.zeros(0, dtype=torch.int32, device=DEV)] * 2
        ctx = attn_fwd(lib, qkv.to(DEV), heads, win if b == 0 else none, ch, tok_lo, p, seed).double().cpu().view(T, heads, 64)
        for s in range(len(lens)):
            a, e, n = int(cu[s]), int(cu[s + 1]), int(lens[s])
            rows = ctx[a:e].permute(1, 0, 2)                                        # (heads, n, 64)
            if is_long[s]:
                k = min(64, n - 64 * b)
                if k <= 0:
                    assert float(rows.abs().max()) == 0.0
                    continue
                raw[s][:, :, 64 * b:64 * b + k] = rows[:, :, :k]
                if k < 64:
                    assert float(rows[:, :, k:].abs().max()) == 0.0, "a probability past the end of a long sequence"
            elif b == 0:
                off = a - win_of[s]
                raw[s][:] = rows[:, :, off:off + n]
                other = rows.clone()
                other[:, :, off:off + n] = 0.0
                assert float(other.abs().max()) == 0.0, "a key of another sequence of the window has a non-zero probability"
    masks, worst = [], 0.0
    for s, n in enumerate(lens):
        r = raw[s] * float(n) * (1.0 - p)                                           # 0 or 1
        keep = r != 0
        if keep.any():
            dev = float((r[keep] - 1.0).abs().max())
            worst = max(worst, dev)
            assert dev <= F16_ROUNDINGS, "sequence %d: a multiplier that is neither 0 nor 1 / (1 - p): off by %.3e" % (s, dev)
        masks.append(keep.double() / (1.0 - p))
    return masks, worst
