"""opt['dp_global_batch'] on the device: W ranks at batch B give the single-process step at batch W * B.
  * world 1 (an in-process RCCL group, as test_gpu_dp.py::test_single_rank_nccl_step_equals_plain_step): the cross-rank layer norm -
    partials, three exchanges, the _global kernels - is bit-identical to the single-tensor op, and so is a whole SDNet step;
  * two ranks (tests/_dp_global_batch_worker.py): over gloo with both ranks on one GPU, and over RCCL with one GPU per rank where the
    box has two: the op against the whole tensor, a B = 8 step against 2 x 4 shards (with the switch-off control), evaluation at
    batch 2 x 2 against one process at batch 4."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ruart_amd import synth                       # noqa: E402
from ruart_amd.arguments import default_opt        # noqa: E402


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.fixture(scope="module")
def world1():
    import datetime
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"), timeout=datetime.timedelta(seconds=120))
    try:
        yield dist.group.WORLD
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("shape", [(64, 100, 250), (64, 36, 250), (64, 40, 250), (3, 7, 13)])
def test_world1_op_bit_identical(world1, shape):
    """Under a world-1 RCCL group the flagged op's y, stats and grad_x are the plain op's bits (the (3, 7, 13) tensor: n % 4 != 0, the
    scalar-tail forms)."""
    from ruart_amd import hip, ops
    from ruart_amd.dp import make_ln_groups
    lib = hip.load()
    g = make_ln_groups(world1)[1]
    gen = torch.Generator().manual_seed(sum(shape))
    x = (torch.randn(*shape, generator=gen) * 2.5 - 0.7).cuda()
    gy = torch.randn(*shape, generator=gen).cuda()
    n = x.numel()
    ws = torch.empty(4096, device="cuda")
    y0, st0, gx0 = torch.empty_like(x), torch.empty(2, device="cuda"), torch.empty_like(x)
    hip.check(lib.ruart_whole_ln_fwd(hip.ptr(x), hip.ptr(y0), hip.ptr(st0), hip.ptr(ws), n, 1e-5, hip.stream_ptr()), "fwd")
    hip.check(lib.ruart_whole_ln_bwd(hip.ptr(y0), hip.ptr(gy), hip.ptr(st0), hip.ptr(gx0), hip.ptr(ws), n, hip.stream_ptr()), "bwd")
    y1, st1 = ops.whole_ln_global_fwd(x, 1e-5, g)
    gx1 = ops.whole_ln_global_bwd(y1, gy, st1, g)
    torch.cuda.synchronize()
    assert torch.equal(y0, y1) and torch.equal(st0, st1) and torch.equal(gx0, gx1)
    # through autograd, both forms of ops.whole_layer_norm
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = ops.whole_layer_norm(xa), ops.whole_layer_norm(xb, group=g)
    ya.backward(gy)
    yb.backward(gy)
    assert torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad) and torch.equal(yb, y0)


def test_world1_model_step_bit_identical(world1):
    """A full SDNet step under the world-1 RCCL group with the switch on: the unflagged step's loss and every gradient, bit for bit
    (the trunk's nine layer norms go through the partials / exchange / _global path)."""
    from ruart_amd.trainer import SDNetTrainer
    opt = default_opt(vocab_size=1500, cuda=True, DROPOUT=0.0, dropout_emb=0.0)
    cfg = synth.bert_config(vocab_size=2000)
    opt["bert_state"], opt["bert_config"] = synth.make_bert_weights(cfg, seed=1033), cfg
    sw = synth.make_sdnet_weights(opt, seed=1033)
    batch = synth.synthetic_batch(opt, 3, seed=5, n_q=10, n_ocr=24, n_od=7, bert_vocab=2000, ragged=True)

    def make(flag):
        tr = SDNetTrainer(dict(opt, dp_global_batch=flag), device="cuda:0", process_group=world1)
        tr.setup_model({"glove_embedding": T(sw["glove_embed.weight"]), "fast_embedding": T(sw["fast_embed.weight"])})
        tr.network.load_state_dict({k: T(v) for k, v in sw.items()})
        assert tr.grad_sync is not None and tr.global_batch == flag
        return tr

    def grads(tr):
        b = tr.ToCUDA(batch)
        tr.network.train()
        tr.network.drop_emb = True
        scores, _ = tr.network(b[0], b[1], b[2])
        loss = tr.loss_func(scores, b[3])
        tr.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        tr.grad_sync.average_gradients()
        torch.cuda.synchronize()
        return loss.item(), {n: p.grad.clone() for n, p in tr.network.named_parameters() if p.grad is not None}

    off, on = make(False), make(True)
    assert off.network.ln_groups() == (None, None, None) and all(g is not None for g in on.network.ln_groups())
    l0, g0 = grads(off)
    l1, g1 = grads(on)
    assert l0 == l1
    assert set(g0) == set(g1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    la = [float(off.update(off.ToCUDA(batch), i)) for i in range(2)]
    lb = [float(on.update(on.ToCUDA(batch), i)) for i in range(2)]
    assert la == lb
    for (n, p), (_, q) in zip(off.network.named_parameters(), on.network.named_parameters()):
        assert torch.equal(p, q), n
    off.close()
    on.close()


def _run_two_ranks(backend, devices, part):
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_dp_global_batch_worker.py")
    port = str(_free_port())
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, worker, str(r), "2", port, backend, str(devices[r]), part], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=420)
            outs.append(out)
    finally:
        for p in procs:                      # exact PIDs of the two children only
            if p.poll() is None:
                p.kill()
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, out[-4000:])
        assert "rank %d ok" % r in out, out[-2000:]


@pytest.mark.parametrize("part", ["op", "model", "eval"])
def test_two_rank_gloo_on_one_gpu(part):
    """Both ranks on cuda:0, collectives on gloo (RCCL refuses two ranks on one device)."""
    _run_two_ranks("gloo", (0, 0), part)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (one RCCL rank per GPU)")
@pytest.mark.parametrize("part", ["op", "model", "eval"])
def test_two_rank_rccl(part):
    _run_two_ranks("nccl", (0, 1), part)
