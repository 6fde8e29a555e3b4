"""CPU companions of the dropout-on GPU tests (tests/test_gpu_train_kernels.py, tests/test_gpu_bert_train_dropout.py): the float64
references of tests/_dropout_ref.py are self-consistent, and every deliberately wrong backward they can restate moves a gradient by
more than three times the bound the GPU tests hold the kernels to - a kernel with that defect cannot pass them.  Synthetic Bernoulli
masks stand in for the ones the GPU tests recover from the kernels."""
import pytest
import torch

from tests import _dropout_ref as R

SEPARATION = 3.0


@pytest.fixture(scope="module")
def attention_cells():
    """family -> p -> (inputs, synthetic masks, float64 gradient of the correct backward); computed once, never written to"""
    cells = {}
    for family in R.ATTN_FAMILIES:
        lens, heads, cu, qkv, dO = R.attention_inputs(family)
        for p in (0.1, 0.5):
            masks = R.bernoulli_masks(torch.Generator().manual_seed(int(p * 100) + len(lens)), p, cu, heads)
            _, want = R.attention_grads(qkv, dO, cu, heads, masks)
            cells[family, p] = (lens, heads, cu, qkv, dO, masks, want)
    return cells


@pytest.mark.parametrize("family", list(R.ATTN_FAMILIES))
def test_written_out_attention_backward_equals_autograd(attention_cells, family):
    lens, heads, cu, qkv, dO, masks, want = attention_cells[family, 0.5]
    out, _ = R.attention_grads(qkv, dO, cu, heads, masks)
    out_plain, plain = R.attention_grads(qkv, dO, cu, heads, masks, plain=True)
    assert torch.equal(out, out_plain)
    assert float((want - plain).abs().max()) < 1e-12 * float(plain.abs().max())
    # without a mask it is the p = 0 reference of tests/test_gpu_train_kernels.py (_attn_ref)
    o1, g1 = R.attention_grads(qkv, dO, cu, heads, None)
    o2, g2 = R.attention_grads(qkv, dO, cu, heads, None, plain=True)
    assert float((o1 - o2).abs().max()) == 0.0 and float((g1 - g2).abs().max()) < 1e-12 * float(g2.abs().max())


@pytest.mark.parametrize("family", list(R.ATTN_FAMILIES))
@pytest.mark.parametrize("mutation", R.ATTN_MUTATIONS)
def test_attention_mutations_are_separated_from_the_gpu_bounds(attention_cells, family, mutation):
    """Each wrong backward moves dQ or dK of some (p, sequence) cell by more than 3x BOTH bounds of the GPU test (max-rel 4e-2, rel-L2
    1.5e-2 per sequence and block), at the lens, heads and dropout probabilities the GPU test runs."""
    heads = R.ATTN_FAMILIES[family][1]
    H = heads * 64
    best = (0.0, 0.0, None)
    for p in (0.1, 0.5):
        lens, heads, cu, qkv, dO, masks, want = attention_cells[family, p]
        _, got = R.attention_grads(qkv, dO, cu, heads, masks, mutation=mutation)
        for s, (a, b) in enumerate(zip(cu[:-1], cu[1:])):
            for name, sl in (("dQ", slice(0, H)), ("dK", slice(H, 2 * H))):
                if float(want[a:b, sl].abs().max()) == 0.0:            # a one-token sequence: P = 1, dS = 0 whatever the mask
                    continue
                e, rel = R.block_errors(got[a:b, sl], want[a:b, sl])
                if min(e / R.ATTN_BOUNDS[0], rel / R.ATTN_BOUNDS[1]) > min(best[0] / R.ATTN_BOUNDS[0], best[1] / R.ATTN_BOUNDS[1]):
                    best = (e, rel, (p, int(b - a), name))
    print("attention mutation %-10s %-6s: max-rel %.3f (bound %.3f), rel-L2 %.3f (bound %.4f) at %s"
          % (mutation, family, best[0], R.ATTN_BOUNDS[0], best[1], R.ATTN_BOUNDS[1], best[2]))
    assert best[0] > SEPARATION * R.ATTN_BOUNDS[0] and best[1] > SEPARATION * R.ATTN_BOUNDS[1], best


# ---- whole encoder ----------------------------------------------------------------------------------------------------------------
ENCODER_BOUND = 3e-2             # rel-L2 per gradient tensor in tests/test_gpu_bert_train_dropout.py


def _synthetic_site_masks(cfg, cu, p, seed):
    g = torch.Generator().manual_seed(seed)
    T, H, nh = int(cu[-1]), int(cfg["hidden_size"]), int(cfg["num_attention_heads"])
    flat = lambda: (torch.rand(T, H, generator=g) >= p).double() / (1.0 - p)
    masks = {"emb": flat()}
    for l in range(int(cfg["num_hidden_layers"])):
        masks["attn", l] = R.bernoulli_masks(g, p, cu, nh)
        masks["ao", l] = flat()
        masks["out", l] = flat()
    return masks


@pytest.fixture(scope="module")
def encoder_cell():
    cfg, state, ids, mask, cu = R.encoder_case()
    params = {k[5:]: torch.from_numpy(v).double() for k, v in state.items() if k.startswith("bert.") and not k.startswith("bert.pooler.")}
    masks = _synthetic_site_masks(cfg, cu, 0.1, 7)
    g_mixed = torch.randn(int(cu[-1]), int(cfg["hidden_size"]), generator=torch.Generator().manual_seed(8)).double()
    ref = R.encoder_reference(cfg, params, ids, mask, cu, g_mixed, masks)
    return cfg, params, ids, mask, cu, g_mixed, masks, ref


def _worst_move(ref, other):
    (_, g0, lw0), (_, g1, lw1) = ref, other
    moves = {n: R.rel_l2(g1[n], g0[n]) for n in g0 if float(g0[n].norm()) > 1e-12 * float(g0["encoder.layer.1.output.dense.weight"].norm())}
    moves["layer_w"] = R.rel_l2(lw1, lw0)
    return moves


def test_encoder_reference_without_masks_is_the_oracle(encoder_cell):
    """No masks: the packed float64 encoder equals oracle.ruart_oracle.bert_forward on the padded batch (the pinned restatement)."""
    from oracle import ruart_oracle as O
    cfg, params, ids, mask, cu, g_mixed, masks, ref = encoder_cell
    lw = torch.tensor(R.ENCODER_LAYER_W, dtype=torch.float64)
    pos = torch.arange(ids.shape[1]).unsqueeze(0).expand_as(ids)[mask]
    with torch.no_grad():
        mine = R.encoder_mixed(params, cfg, ids[mask], pos, cu, lw, {})
        # float64 weights: the oracle's fp32 key-mask constant is promoted; masked keys get exp(-10000) == 0 either way
        layers = O.bert_forward({"bert." + n: t for n, t in params.items()}, cfg, ids, mask.double())
    want = sum(w * l[mask] for w, l in zip(R.ENCODER_LAYER_W, layers))
    assert float((mine - want).abs().max()) < 1e-9


def test_encoder_mask_mixups_are_separated_from_the_gpu_bound(encoder_cell):
    """(e) the backward of one layer regenerates the masks of its two dense-output sites the wrong way round (forward right), and
    layer 1 drawing layer 0's attention-probability mask: each moves at least one gradient tensor by more than 3x the rel-L2 bound of
    the GPU test."""
    cfg, params, ids, mask, cu, g_mixed, masks, ref = encoder_cell
    smallest = None
    for l in range(int(cfg["num_hidden_layers"])):
        swapped = {("ao", l): masks["out", l], ("out", l): masks["ao", l]}
        moves = _worst_move(ref, R.encoder_reference(cfg, params, ids, mask, cu, g_mixed, masks, bwd_masks=swapped))
        name = max(moves, key=moves.get)
        print("encoder mutation (e), layer %d: %d of %d tensors move by more than %.2f; largest %.3f (%s)"
              % (l, sum(v > SEPARATION * ENCODER_BOUND for v in moves.values()), len(moves), SEPARATION * ENCODER_BOUND, moves[name], name))
        assert moves[name] > SEPARATION * ENCODER_BOUND, (l, name, moves[name])
        smallest = moves[name] if smallest is None else min(smallest, moves[name])
    wrong = dict(masks)
    wrong["attn", 1] = masks["attn", 0]
    moves = _worst_move(ref, R.encoder_reference(cfg, params, ids, mask, cu, g_mixed, wrong))
    name = max(moves, key=moves.get)
    print("encoder mutation 'layer 1 draws layer 0's attention mask': %d of %d tensors move by more than %.2f; largest %.3f (%s)"
          % (sum(v > SEPARATION * ENCODER_BOUND for v in moves.values()), len(moves), SEPARATION * ENCODER_BOUND, moves[name], name))
    assert moves[name] > SEPARATION * ENCODER_BOUND, (name, moves[name])
    print("smallest of the largest moves: %.3f" % min(smallest, moves[name]))


def test_mask_statistics_helpers():
    g = torch.Generator().manual_seed(3)
    a = torch.rand(200000, generator=g) >= 0.1
    b = torch.rand(200000, generator=g) >= 0.1
    assert R.keep_sigmas(a, 0.1) < 5 and R.agree_sigmas(a, b, 0.1) < 5
    assert R.agree_sigmas(a, a, 0.1) > 50                                 # the same stream
    assert R.shifted_agree_sigmas(torch.cat([a[7:], b[:7]]), a, 7, 0.1) < 5 < R.shifted_agree_sigmas(torch.cat([a[7:], b[:7]]), a, -7, 0.1)
    assert R.shifted_agree_sigmas(a, b, 200000, 0.1) is None
