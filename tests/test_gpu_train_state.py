"""A resumed run IS the uninterrupted run, bit for bit (``SDNetTrainer.save`` / ``load_state``, opt['save_every'] / opt['resume_state']),
under the real schedule: the encoder pass one step ahead on its own stream, three trunk streams, the loss read back one step late.

Straight arm: six ``update(batch_i, i, next_batch=batch_{i+1})`` calls.  Resumed arm: three such calls, ``save``, ``close()``, a new
trainer, ``setup_model``, ``load_state``, the remaining three.  The save falls on an odd update count (the fused step alternates two
staging buffers by ``step_count & 1``).  Everything is compared with ``torch.equal`` / ``==``: the losses of steps 3-5, every named
parameter, every optimizer state tensor and per-tensor step count, ``updates``, ``train_loss.avg``, the final CPU and device generator
states.  Two controls keep the comparison from passing vacuously: resuming the weights only, and resuming everything but the
generators' position, must both differ."""
import copy
import functools
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ruart_amd import layers as L                         # noqa: E402
from ruart_amd import synth                               # noqa: E402
from ruart_amd.arguments import default_opt               # noqa: E402

DEV = "cuda:0"
STEPS, CUT = 6, 3


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def _bert():
    """(synthetic bert-base checkpoint, its config: both dropouts 0.1) - built once per module and never written to"""
    cfg = synth.bert_config(vocab_size=2000)
    assert cfg["hidden_dropout_prob"] == 0.1 and cfg["attention_probs_dropout_prob"] == 0.1
    return synth.make_bert_weights(cfg, seed=7, w_std=0.02), cfg


def _opt(conf, **extra):
    """'shipped': the shipped conf with its dropouts on (frozen encoder running ahead, TUNE_PARTIAL);  'trained': the top two encoder
    layers trained on the 16-bit kernels as an AdamW group of their own, warm-up over the first half of six steps"""
    opt = default_opt(vocab_size=600, cuda=True)
    assert float(opt["DROPOUT"]) == 0.3 and float(opt["dropout_emb"]) == 0.4 and "TUNE_PARTIAL" in opt and "LOCK_BERT" in opt
    if conf == "trained":
        opt.pop("LOCK_BERT")
        opt.update(bert_train_gemm="16", bert_train_layers=2, bert_optimizer="adamw", bert_warmup=0.5, bert_t_total=6)
    opt.update(extra)
    opt["bert_state"], opt["bert_config"] = _bert()
    return opt


@functools.lru_cache(maxsize=None)
def _host_batches():
    opt = _opt("shipped")
    return [synth.synthetic_batch(opt, 3, seed=31 + i, n_q=10, n_ocr=14, n_od=5, bert_vocab=2000, ragged=True) for i in range(STEPS)]


@functools.lru_cache(maxsize=None)
def _embeddings():
    sw = synth.make_sdnet_weights(_opt("shipped"), seed=7)
    return {"glove_embedding": T(sw["glove_embed.weight"]), "fast_embedding": T(sw["fast_embed.weight"])}


def _trainer(opt):
    """A new trainer; its weights come from the conf's SEED (the constructor seeds every generator), so two of them start alike."""
    from ruart_amd.trainer import SDNetTrainer
    tr = SDNetTrainer(dict(opt), device=DEV)
    tr.setup_model(_embeddings())
    return tr, [tr.ToCUDA(b) for b in copy.deepcopy(_host_batches())]


def _run(tr, batches, lo, hi):
    """update() for batches lo .. hi-1, the next batch's encoder pass running ahead; deferred losses are resolved at the end"""
    losses = [tr.update(batches[i], i, next_batch=batches[i + 1] if i + 1 < len(batches) else None) for i in range(lo, hi)]
    return [float(x) for x in losses]


def _optimizer_state(tr):
    o, out = tr.optimizer, {}
    # (the project's optimizers key their state by id(parameter), torch's by the tensor)
    st = {(id(k) if torch.is_tensor(k) else k): v for k, v in o.state.items()}
    for n, p in tr.network.named_parameters():
        ent = st.get(id(p), {})
        for k, v in ent.items():
            out["%s.%s" % (n, k)] = v.detach().cpu().clone() if torch.is_tensor(v) else v
        if hasattr(o, "steps") and id(p) in o.steps:
            out[n + ".steps"] = o.steps[id(p)]
    if hasattr(o, "step_count"):
        out["step_count"] = o.step_count
    return out


def _snapshot(tr, losses):
    tr.flush_readback()
    torch.cuda.synchronize()
    return {"losses": losses, "params": {n: p.detach().cpu().clone() for n, p in tr.network.named_parameters()},
            "optimizer": _optimizer_state(tr), "updates": tr.updates, "avg": tr.train_loss.avg, "count": tr.train_loss.count,
            "cpu_rng": torch.get_rng_state().clone(), "cuda_rng": torch.cuda.get_rng_state(torch.device(DEV)).clone(),
            "best": (tr.best_ANLS, tr.best_ACC, tr.best_ANLS_batch, tr.best_ACC_batch)}


def _differences(a, b):
    bad = []
    for k in ("losses", "updates", "avg", "count", "best"):
        if a[k] != b[k]:
            bad.append("%s: %r vs %r" % (k, a[k], b[k]))
    for k in ("cpu_rng", "cuda_rng"):
        if not torch.equal(a[k], b[k]):
            bad.append(k)
    for group in ("params", "optimizer"):
        if set(a[group]) != set(b[group]):
            bad.append("%s: different keys" % group)
            continue
        for n, v in a[group].items():
            w = b[group][n]
            if not (torch.equal(v, w) if torch.is_tensor(v) else v == w):
                bad.append("%s %s" % (group, n))
    return bad


@pytest.fixture(scope="module")
def state_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("train_state"))


@functools.lru_cache(maxsize=None)
def _straight(conf, fused):
    """The uninterrupted run: computed once, shared by the tests that compare against it, never changed."""
    L.mask_bank = L.MaskBank()
    tr, batches = _trainer(_opt(conf, ruart_fused_optimizer=fused))
    try:
        return _snapshot(tr, _run(tr, batches, 0, STEPS))
    finally:
        tr.close()


@functools.lru_cache(maxsize=None)
def _first_half(conf, fused, folder):
    """Three steps, then ``save`` and ``close``; returns the file.  Shared by the resumed arm and the controls."""
    L.mask_bank = L.MaskBank()
    tr, batches = _trainer(_opt(conf, ruart_fused_optimizer=fused))
    path = os.path.join(folder, "%s_%d.pt" % (conf, fused))
    try:
        _run(tr, batches, 0, CUT)
        assert tr.updates % 2 == 1 and getattr(tr.optimizer, "step_count", CUT) == CUT        # an odd count: the other staging buffer next
        prev = path + ".prev"
        open(prev, "w").close()
        tr.save(path, epoch=0, prev_filename=prev)
        assert os.path.exists(path) and not os.path.exists(prev)
        assert not [f for f in os.listdir(folder) if ".tmp" in f]                             # the temporary name is gone
    finally:
        tr.close()
    return path


def _second_half(conf, fused, path, how):
    """A new trainer continues from ``path``.  how = 'state': load_state;  'weights': load_model, the reference's way;  'reseed': load_state,
    then the generators are seeded anew."""
    tr, batches = _trainer(_opt(conf, ruart_fused_optimizer=fused))
    try:
        if how == "weights":
            tr.load_model(path)
            tr.updates = CUT
        else:
            L.mask_bank.demand, L.mask_bank.used = {0.4: 12345}, {0.4: 99}      # an earlier trainer's leftovers: replaced, not merged
            assert tr.load_state(path) == CUT
            assert L.mask_bank.used == {} and L.mask_bank.buf == {} and 12345 not in L.mask_bank.demand.values()
        if how == "reseed":
            torch.manual_seed(12345)
        return _snapshot(tr, _run(tr, batches, CUT, STEPS))
    finally:
        tr.close()


def _check_resumed(conf, fused, state_dir):
    want = _straight(conf, fused)
    path = _first_half(conf, fused, state_dir)
    got = _second_half(conf, fused, path, "state")
    assert all(x == x for x in want["losses"])
    print("straight losses %s; resumed %s" % (want["losses"], got["losses"]))
    got = dict(got, losses=want["losses"][:CUT] + got["losses"])
    bad = _differences(want, got)
    assert not bad, "%d differences between the resumed and the uninterrupted run, e.g. %s" % (len(bad), bad[:6])
    assert want["updates"] == STEPS and want["count"] == STEPS and len(want["optimizer"]) > 50
    return path


@pytest.mark.parametrize("fused", [True, False])
def test_shipped_conf_resumes_bit_for_bit(fused, state_dir):
    """Conf 1: DROPOUT 0.3, dropout_emb 0.4, TUNE_PARTIAL, frozen encoder one step ahead; FusedAdamax / torch.optim.Adamax."""
    from ruart_amd.optim import FusedAdamax
    path = _check_resumed("shipped", fused, state_dir)
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    assert ckpt["ruart"]["optimizer_class"] == ("FusedAdamax" if fused else "Adamax") == (FusedAdamax if fused else torch.optim.Adamax).__name__
    net = ckpt["state_dict"]["network"]
    assert "alphaBERT" in net and "fast_embed.weight" in net and not [k for k in net if k.startswith("Bert.")]     # frozen: from BERT_model_file again
    assert ckpt["state_dict"]["updates"] == CUT and ckpt["ruart"]["next_batch"] == CUT and ckpt["epoch"] == 0
    assert len(ckpt["ruart"]["ranks"]) == 1 and set(ckpt["ruart"]["ranks"][0]["banks"]) == {"front", "trunk"}
    assert all(n > 0 for bank in ckpt["ruart"]["ranks"][0]["banks"].values() for _, n in bank)
    assert "bert_state" not in ckpt["config"] and ckpt["config"]["DROPOUT"] == 0.3


def test_trained_encoder_resumes_bit_for_bit(state_dir):
    """Conf 2: the top two encoder layers trained (16-bit kernels, BERT dropouts 0.1 drawn from a per-pass seed of the CPU generator),
    AdamW group with warm-up - its position is the per-tensor step counts -, readback deferred (the default there)."""
    from ruart_amd.optim import FusedAdamaxAdam
    path = _check_resumed("trained", True, state_dir)
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    assert ckpt["ruart"]["optimizer_class"] == FusedAdamaxAdam.__name__ and ckpt["ruart"]["optimizer_rule"] == "adamw"
    enc = [k for k in ckpt["state_dict"]["network"] if k.startswith("Bert.bert_model.")]
    assert enc and all(".layer.10." in k or ".layer.11." in k or ".pooler." in k for k in enc)
    assert max(ckpt["state_dict"]["optimizer"]["steps"]) == CUT
    want = _straight("trained", True)
    w11 = "Bert.bert_model.encoder.layer.11.output.dense.weight"
    assert want["optimizer"][w11 + ".steps"] == STEPS and float(want["optimizer"][w11 + ".exp_avg_sq"].abs().max()) > 0


def test_control_weights_only_resume_differs(state_dir):
    """Resumed the reference's way - ``load_model`` on the same file, a fresh optimizer: Adamax with zeroed moments takes other steps."""
    want = _straight("shipped", True)
    got = _second_half("shipped", True, _first_half("shipped", True, state_dir), "weights")
    assert [n for n in want["params"] if not torch.equal(want["params"][n], got["params"][n])]


def test_control_reseeded_resume_differs(state_dir):
    """A full ``load_state`` followed by ``torch.manual_seed``: other masks at p = 0.3 / 0.4, other losses."""
    want = _straight("shipped", True)
    got = _second_half("shipped", True, _first_half("shipped", True, state_dir), "reseed")
    assert got["losses"] != want["losses"][CUT:], (got["losses"], want["losses"])


def test_refusals_on_the_trainer(state_dir):
    from ruart_amd.trainer import SDNetTrainer
    path = _first_half("shipped", True, state_dir)
    tr, _ = _trainer(_opt("shipped", ruart_fused_optimizer=False))
    try:
        with pytest.raises(ValueError, match="optimizer class FusedAdamax.*Adamax"):
            tr.load_state(path)
        tr.opt["ruart_graph_trunk"] = True
        with pytest.raises(ValueError, match="ruart_graph_trunk"):
            tr.save(os.path.join(state_dir, "never.pt"))
        with pytest.raises(ValueError, match="ruart_graph_trunk"):
            tr.load_state(path)
        tr.opt.pop("ruart_graph_trunk")
        for key in ("save_every", "resume_state"):
            t2 = SDNetTrainer(dict(_opt("shipped", ruart_graph_trunk=True), **{key: 3 if key == "save_every" else path}), device=DEV)
            with pytest.raises(ValueError, match="ruart_graph_trunk"):
                t2.train([], None)
        t3 = SDNetTrainer(dict(_opt("shipped"), resume_state=path, batch_st=1), device=DEV)
        with pytest.raises(ValueError, match="batch_st.*continues at batch 3"):
            t3.train([], None)
        assert not os.path.exists(os.path.join(state_dir, "never.pt"))
    finally:
        tr.close()


def test_train_saves_and_resumes(golden_dir, tmp_path):
    """Conf 3, through ``train()``: six collated batches, a ``VQA_Dataset`` evaluated every three.  Without the keys no train_state.pt
    is written; ``save_every = 3`` leaves one after the third update without changing the run; a second trainer with ``resume_state``
    and the last three batches ends bit-equal to the straight run, and its first evaluation - ANLS no higher than the best on record -
    leaves ANLS_best_model.pt alone."""
    from ruart_amd.dataset import VQA_Dataset
    from ruart_amd.trainer import SDNetTrainer
    with open(os.path.join(golden_dir, "dataset_input.json"), encoding="utf-8") as f:
        inp = json.load(f)
    vocab = tmp_path / "vocab.txt"
    vocab.write_text("\n".join(inp["vocab"]) + "\n", encoding="utf-8")
    base = default_opt(datadir="", BERT_tokenizer_file=str(vocab), cuda=True, batch_size=4)
    base["bert_state"], base["bert_config"] = _bert()
    sw = synth.make_sdnet_weights(base, seed=7)
    emb = {"glove_embedding": T(sw["glove_embed.weight"]), "fast_embedding": T(sw["fast_embed.weight"])}
    host = [synth.synthetic_batch(base, 3, seed=31 + i, n_q=10, n_ocr=14, n_od=5, bert_vocab=2000, ragged=True) for i in range(STEPS)]
    val = VQA_Dataset(copy.deepcopy(inp["records"]), base, mode="dev")

    def arm(folder, batches, **keys):
        L.mask_bank = L.MaskBank()
        os.makedirs(folder, exist_ok=True)
        tr = SDNetTrainer(dict(base, saveFolder=folder, **keys), device=DEV)
        tr.setup_model(emb)
        return tr, copy.deepcopy(batches)

    fa, fb, fc = (str(tmp_path / n) for n in ("straight", "saving", "resumed"))
    tr, batches = arm(fa, host)
    tr.train(batches, val, eval_every=3, log_every=2)
    straight = _snapshot(tr, [])
    assert tr.updates == STEPS and os.path.exists(os.path.join(fa, "ANLS_best_model.pt"))
    assert not os.path.exists(os.path.join(fa, "train_state.pt"))

    tr, batches = arm(fb, host, save_every=3)
    saves, save = [], tr.save

    def spy(filename, *a, **kw):
        save(filename, *a, **kw)
        saves.append((filename, tr.updates))
        if len(saves) == 1:                      # the run folder as a job cut off here would leave it
            shutil.copytree(fb, fc)
    tr.save = spy
    tr.train(batches, val, eval_every=3, log_every=2)
    assert saves == [(os.path.join(fb, "train_state.pt"), 3), (os.path.join(fb, "train_state.pt"), 6)]
    bad = _differences(straight, _snapshot(tr, []))
    assert not bad, "saving changed the run: %s" % bad[:6]

    best_file = os.path.join(fc, "ANLS_best_model.pt")
    state_file = os.path.join(fc, "train_state.pt")
    assert os.path.exists(best_file) and torch.load(state_file, weights_only=True)["ruart"]["best"]["ANLS_batch"] == 0
    with open(best_file, "wb") as f:
        f.write(b"sentinel")
    tr, batches = arm(str(tmp_path / "unused"), host[CUT:], resume_state=state_file, save_every=3)
    assert tr.best_ANLS == -1
    tr.train(batches, val, eval_every=3, log_every=2)
    assert tr.saveFolder == fc and not os.listdir(str(tmp_path / "unused")) and not os.path.exists(os.path.join(fc, "conf_copy"))
    bad = _differences(straight, _snapshot(tr, []))
    assert not bad, "%d differences between the resumed and the uninterrupted train(), e.g. %s" % (len(bad), bad[:6])
    assert tr.best_ANLS == straight["best"][0] >= 0
    rewritten = open(best_file, "rb").read() != b"sentinel"
    assert rewritten == (straight["best"][2] == CUT), (rewritten, straight["best"])
    assert torch.load(state_file, weights_only=True)["ruart"]["next_batch"] == STEPS


def _launch_two_ranks(phase, folder):
    """Two children on cuda:0 over gloo (with this process three hold the GPU), each under its own time limit; exit codes asserted,
    nothing retried."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_train_state_two_rank_worker.py")
    rdzv = os.path.join(folder, "rendezvous_" + phase)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, worker, str(r), "2", rdzv, "gloo", "0", phase, folder], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=300)
            outs.append(out)
    finally:
        for p in procs:                      # exact PIDs of the two children only
            if p.poll() is None:
                p.kill()
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d failed in phase %s:\n%s" % (r, phase, out[-4000:])
        assert "rank %d ok" % r in out, out[-2000:]


def test_two_ranks_resume_bit_for_bit(tmp_path):
    """Conf 4: two ranks on one GPU over gloo, a different shard per rank, dropout on; save after two steps, fresh processes resume
    for two more.  Both ranks' parameters equal the uninterrupted two-rank run's, and each other's."""
    folder = str(tmp_path)
    _launch_two_ranks("first", folder)
    ckpt = torch.load(os.path.join(folder, "train_state.pt"), map_location="cpu", weights_only=True)
    ranks = ckpt["ruart"]["ranks"]
    assert ckpt["ruart"]["world"] == 2 and len(ranks) == 2 and ckpt["ruart"]["next_batch"] == 2
    assert not torch.equal(ranks[0]["streams"]["torch_cuda"], ranks[1]["streams"]["torch_cuda"])      # SEED + 7919 r
    _launch_two_ranks("second", folder)
    files = {n: torch.load(os.path.join(folder, n + ".pt"), map_location="cpu", weights_only=True)
             for n in ("straight_r0", "straight_r1", "resumed_r0", "resumed_r1")}
    want = files["straight_r0"]
    assert want["updates"] == 4 and len(want["params"]) > 50
    for n, f in files.items():
        assert f["updates"] == 4, n
        bad = [k for k in want["params"] if not torch.equal(want["params"][k], f["params"][k])]
        assert not bad, "%s: %d of %d parameters differ from the uninterrupted run's, e.g. %s" % (n, len(bad), len(want["params"]), bad[:3])
