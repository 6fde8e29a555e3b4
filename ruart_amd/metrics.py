"""Answer-string metrics used by ``SDNetTrainer.predict`` (restated from Utils/eval_func.py:1-35, 62-68).

``stvqa_score`` / ``note_stvqa`` / ``note_textvqa`` are host string work: the CPU path, and the reference of everything below.
``answer_table`` scores EVERY candidate of a batch against every answer of its sample on the GPU (``ruart_edit_distance_pairs``,
csrc/answer_metrics.hip): the decode of ``predict`` reads the chosen slot's two values out of it, ``opt['eval_upper_bound']`` takes its
row maxima and ``opt['label_from_answers']`` builds training targets from it (``labels_from_table``).  The table is bit-equal to the
host functions: the kernel returns integers, and ``1 - ld / max(len)`` in float64 on the device is the same two correctly rounded
operations Python performs."""
import numpy as np
import torch

EDIT_MAX_LEN = 128          # RUART_EDIT_MAX_LEN (include/ruart_hip.h): longer strings are scored on the host and patched in
NOREAD = "answering does not require reading text in the image"
FRONT_ANSWERS = (NOREAD, "yes", "no")         # the three front slots of ``label_yesno``, in slot order


def stvqa_score(a, b):
    """1 - Levenshtein(a, b) / max(len): the ANLS per-pair score."""
    a, b = a.lower(), b.lower()
    if max(len(a), len(b)) == 0:
        return 1
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return 1 - prev[-1] / max(len(a), len(b))


def note_stvqa(gt_list, word):
    return max([stvqa_score(gt, word) for gt in gt_list] + [-1])


def note_textvqa(gt_list, word):
    return sum(1 for gt in gt_list if gt.lower() == word) / 10.0


# -- the table on the GPU ------------------------------------------------------------------------------------------------
def pack_strings(strings):
    """Strings -> (code points int32 (n_chars,), offsets int32 (len(strings) + 1,)): ONE encode of the joined text and a length list
    (``len(str)`` counts code points, which is what UTF-32 holds one of per unit; lone surrogates pass through as their own value)."""
    n = len(strings)
    off = np.zeros(n + 1, dtype=np.int32)
    if n:
        np.cumsum(np.fromiter(map(len, strings), dtype=np.int64, count=n), out=off[1:])
    chars = np.frombuffer("".join(strings).encode("utf-32-le", "surrogatepass"), dtype="<i4")
    return chars, off


_SECTIONS = ("chars", "off", "pair_a", "pair_b", "flat", "maxlen", "flag")


def pack_answer_table(candidates, answers):
    """The host half of ``answer_table``: lower-case (Python's own ``str.lower()``, which can change a string's length), pack, and
    list the (candidate, answer) pairs of every sample.  Returns a dict of tensors and ints - one int32 buffer holds everything the
    device needs, so it crosses in one copy (and is pinned with the batch when a DataLoader built it) - for ``answer_table_from_pack``.
    Pairs with a string of more than EDIT_MAX_LEN code points are scored here with ``stvqa_score`` and travel as patches."""
    B = len(candidates)
    answers = [a if a is not None else () for a in answers]
    n_c = np.fromiter((len(c) for c in candidates), dtype=np.int64, count=B)
    n_a = np.fromiter((len(a) for a in answers), dtype=np.int64, count=B)
    Cmax, Amax = int(n_c.max()) if B else 0, int(n_a.max()) if B else 0
    raw = [w for c in candidates for w in c]
    low = [w.lower() for w in raw]
    n_cand = len(low)
    strings = low + [g.lower() for a in answers for g in a]
    chars, off = pack_strings(strings)
    lens = np.diff(off).astype(np.int64)
    c_base, a_base = np.cumsum(n_c) - n_c, n_cand + np.cumsum(n_a) - n_a
    # candidate flags, (B, Cmax) flattened: 1 = a real candidate, 2 = ``word == word.lower()`` (note_textvqa lower-cases the answers,
    # not the word: any other word counts 0)
    flag = np.zeros(B * Cmax, dtype=np.int32)
    if n_cand:
        sample_of = np.repeat(np.arange(B), n_c)
        slot_of = np.arange(n_cand) - np.repeat(c_base, n_c)
        flag[sample_of * Cmax + slot_of] = 1 + 2 * np.fromiter((w == l for w, l in zip(raw, low)), dtype=np.int64, count=n_cand)
    # the pairs of sample b: candidate i x answer k, i-major
    n_p = n_c * n_a
    P = int(n_p.sum())
    pb = np.repeat(np.arange(B), n_p)
    r = np.arange(P) - np.repeat(np.cumsum(n_p) - n_p, n_p)
    ci, ai = r // np.maximum(n_a[pb], 1), r % np.maximum(n_a[pb], 1)
    pair_a, pair_b = c_base[pb] + ci, a_base[pb] + ai
    flat = (pb * Cmax + ci) * Amax + ai
    maxlen = np.maximum(lens[pair_a], lens[pair_b])
    patch = None
    over = maxlen > EDIT_MAX_LEN
    if over.any():
        idx = np.nonzero(over)[0]
        sc = [stvqa_score(strings[pair_b[p]], strings[pair_a[p]]) for p in idx]
        eq = [int(strings[pair_b[p]] == strings[pair_a[p]]) for p in idx]
        patch = (torch.from_numpy(flat[idx]), torch.tensor(sc, dtype=torch.float64), torch.tensor(eq, dtype=torch.int32))
        keep = ~over
        pair_a, pair_b, flat, maxlen = pair_a[keep], pair_b[keep], flat[keep], maxlen[keep]
        P = int(keep.sum())
    parts = (chars, off, pair_a, pair_b, flat, maxlen, flag)
    buf = np.concatenate([np.asarray(p, dtype=np.int32) for p in parts]) if B else np.zeros(1, dtype=np.int32)
    return {"buf": torch.from_numpy(buf), "sizes": tuple(int(len(p)) for p in parts), "n_pairs": P, "B": B, "Cmax": Cmax,
            "Amax": Amax, "patch": patch}


def answer_table_from_pack(pack, device):
    """The device half: upload, one ``ruart_edit_distance_pairs`` launch, and the finish in float64 - ``1 - ld / max(len)`` (1 when
    both strings are empty), the maximum over a sample's answers with the reference's -1 beside it, the count of equal pairs over
    ten.  -> (anls, acc), float64 (B, Cmax) on ``device``; padding 0."""
    from . import hip
    device = torch.device(device)
    if device.type != "cuda":
        raise hip.HipError("answer_table runs on the GPU (got device %s); note_stvqa / note_textvqa are the host path" % device)
    B, Cmax, Amax, P = pack["B"], pack["Cmax"], pack["Amax"], pack["n_pairs"]
    with torch.cuda.device(device):
        buf = pack["buf"].to(device, non_blocking=True)
        sec, o = {}, 0
        for name, n in zip(_SECTIONS, pack["sizes"]):
            sec[name] = buf[o:o + n]
            o += n
        score = torch.full((B * Cmax * Amax,), -1.0, dtype=torch.float64, device=device)
        same = torch.zeros(B * Cmax * Amax, dtype=torch.int32, device=device)
        if P:
            dist = torch.empty(P, dtype=torch.int32, device=device)
            eq = torch.empty(P, dtype=torch.int32, device=device)
            hip.kernels().ruart_edit_distance_pairs(sec["chars"], len(sec["chars"]), sec["off"], len(sec["off"]) - 1, sec["pair_a"],
                                                    sec["pair_b"], P, dist, eq, hip.stream_ptr(device))
            ml = sec["maxlen"]
            one = torch.ones((), dtype=torch.float64, device=device)
            flat = sec["flat"].long()
            score[flat] = torch.where(ml == 0, one, 1 - dist.double() / ml.double().clamp(min=1))
            same[flat] = eq
        if pack["patch"] is not None:
            pf, ps, pe = (t.to(device, non_blocking=True) for t in pack["patch"])
            score[pf] = ps
            same[pf] = pe
        flag = sec["flag"].view(B, Cmax)
        floor = torch.full((B, Cmax, 1), -1.0, dtype=torch.float64, device=device)      # note_stvqa: max(scores + [-1])
        anls = torch.cat([score.view(B, Cmax, Amax), floor], dim=2).max(dim=2).values
        anls = torch.where(flag > 0, anls, torch.zeros_like(anls))
        # (a TENSOR divisor: torch divides a device tensor by a python scalar as a product with its reciprocal, which is not the
        # correctly rounded quotient - 3 / 10.0 came out as 0.30000000000000004)
        acc = same.view(B, Cmax, Amax).sum(dim=2).double() / torch.full((), 10.0, dtype=torch.float64, device=device)
        acc = torch.where(flag == 3, acc, torch.zeros_like(acc))
    return anls, acc


def answer_table(candidates, answers, device="cuda"):
    """``candidates``: per sample a list of strings; ``answers``: per sample a list of strings or None.  -> (anls, acc), float64
    (B, Cmax) tensors on ``device``: anls[b, i] is bit-equal to ``note_stvqa(answers[b], candidates[b][i])`` and acc[b, i] to
    ``note_textvqa(answers[b], candidates[b][i])`` (-1 and 0.0 for a sample without answers); padding is 0."""
    return answer_table_from_pack(pack_answer_table(candidates, answers), device)


# -- training targets from the table (opt['label_from_answers']) ------------------------------------------------------------
def label_candidates(extra_info, opt):
    """Per sample the strings ``VQA_Dataset.get_label`` has scores for: the three front answers under ``label_yesno``, then the
    sample's OCR strings WITHOUT the trailing ``<OCR>`` sentinel (whose score is 0.0 by construction, not a string score)."""
    front = list(FRONT_ANSWERS) if "label_yesno" in opt else []
    return [front + list(e["ocr_list"][:-1]) for e in extra_info]


def pack_label_table(extra_info, opt):
    """What ``VQA_collate`` attaches for a batch without host labels: the packed table of ``label_candidates`` against the answers."""
    cands = label_candidates(extra_info, opt)
    pack = pack_answer_table(cands, [e["answers"] for e in extra_info])
    pack["n_scored"] = torch.tensor([len(c) for c in cands], dtype=torch.int64)
    return pack


def labels_from_table(table, n_scored, opt):
    """``VQA_Dataset.get_label`` restated for tensors.  ``table`` (B, C) float64: row b holds the ``opt['score_name']`` scores of
    sample b's ``n_scored[b]`` strings (front answers, then OCR strings); the sentinel's 0.0 follows them, the rest is padding.
    -> float32 (B, n_front + max_ocr_num (+ 1 with ``label_no_answer``)) on the table's device."""
    B, dev = table.shape[0], table.device
    width = (3 if "label_yesno" in opt else 0) + opt["max_ocr_num"]
    n = torch.as_tensor(n_scored, device=dev).view(B, 1)
    if table.shape[1] >= width:                              # (n_scored <= table.shape[1]: no readback needed to know that it fits)
        raise ValueError("labels_from_table: %d scored strings do not fit %d slots with the sentinel" % (table.shape[1], width))
    ar = torch.arange(width, device=dev).view(1, width)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    gt = torch.zeros(B, width, dtype=torch.float64, device=dev)
    gt[:, :table.shape[1]] = table
    gt = torch.where(ar < n, gt, zero)                       # the sentinel's 0.0 at slot n, zeros behind it
    listed = ar <= n
    masked = torch.where(listed, gt, torch.full_like(gt, float("-inf")))
    best = masked.max(dim=1, keepdim=True).values
    # the FIRST maximum, as the reference's ``t > best`` walk from -1 finds it (no slot when nothing exceeds -1)
    first = torch.where(masked == best, ar, torch.full_like(ar, width)).min(dim=1, keepdim=True).values
    best_idx = torch.where(best > -1, first, torch.full_like(first, -1))
    way = opt["lable_way"]
    if way == "lable_all_with_threshold":
        gt = torch.where(gt >= opt["score_threshold"], gt, zero)
    elif way == "lable_one_offical":
        floor = {"ANLS": 0.5, "ACC": 0.3}.get(opt["score_name"])
        if floor is not None:
            gt = torch.where((ar == best_idx) & (best >= floor), gt, zero)
    elif way == "lable_one":
        gt = torch.where(ar == best_idx, gt, zero)
    elif way != "lable_all":
        raise AssertionError("lable_way is wrong")
    out = torch.where(listed, gt, zero).to(torch.float32)
    if "label_no_answer" in opt:
        out = torch.cat([out, (best < 0.1).to(torch.float32)], dim=1)
    return out


def labels_from_pack(pack, opt, device):
    """``SDNetTrainer.ToCUDA``: the targets of a batch that came without host labels."""
    if opt["score_name"] not in ("ANLS", "ACC"):
        raise ValueError("opt['label_from_answers'] scores ANLS or ACC, not opt['score_name'] = %r" % (opt["score_name"],))
    anls, acc = answer_table_from_pack(pack, device)
    return labels_from_table(anls if opt["score_name"] == "ANLS" else acc, pack["n_scored"].to(device, non_blocking=True), opt)
