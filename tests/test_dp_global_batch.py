"""opt['dp_global_batch'] on the host: the sharded evaluation stream gathered back into one process's order, and the switch's
refusals.  (The kernels, the exchanges and the trainer on the device: tests/test_gpu_dp_global_batch.py.)"""
import pytest

from ruart_amd.arguments import default_opt
from ruart_amd.sampler import VQA_Sampler, merge_rank_shards


class _Records:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("n_items", [1, 7, 29, 53])
def test_merge_rank_shards_is_the_single_process_order(world, n_items):
    """W ranks at batch B, each predicting global[r::W] of every global batch, merge into exactly what one process at batch W * B
    walks (wrap-around of the last batch included); the test-mode trim by the global batch size leaves every record once, in order."""
    B = 2
    data = _Records(n_items)
    single = [i for b in VQA_Sampler(data, None, world * B, False) for i in b]
    per_rank = [[i for b in VQA_Sampler(data, None, B, False, rank=r, world_size=world) for i in b] for r in range(world)]
    assert n_items % (world * B) != 0 or n_items == 0
    assert all(len(p) == len(per_rank[0]) for p in per_rank)
    merged = merge_rank_shards(per_rank, B)
    assert merged == single
    # the same walk with per-sample result records instead of indices (what _evaluate gathers)
    recs = [[{"question_id": i, "answer": "a%d" % i} for i in p] for p in per_rank]
    assert [r["question_id"] for r in merge_rank_shards(recs, B)] == single
    gb = world * B
    end = n_items % gb
    trimmed = merged[:-(gb - end)] if end else merged
    assert trimmed == list(range(n_items))


def test_merge_rank_shards_refuses_unequal_shards():
    with pytest.raises(ValueError):
        merge_rank_shards([[0, 1], [2]], 2)
    with pytest.raises(ValueError):
        merge_rank_shards([[0, 1, 2], [3, 4, 5]], 2)


@pytest.mark.parametrize("other", ["dp_overlap_backward", "ruart_graph_trunk"])
def test_switch_refuses_incompatible_modes(other):
    """opt['dp_global_batch'] with the hook-time gradient exchange or the captured trunk is an error (before any model is built);
    without the switch neither option is refused here."""
    from ruart_amd.trainer import SDNetTrainer
    opt = default_opt(vocab_size=100, cuda=False, dp_global_batch=True)
    opt[other] = True
    tr = SDNetTrainer(opt, device="cpu")
    with pytest.raises(ValueError, match="dp_global_batch"):
        tr.setup_model(None)
