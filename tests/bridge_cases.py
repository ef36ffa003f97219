"""Seeded inputs of tests/test_bridge_kernel_gpu.py.  TEST INFRASTRUCTURE, shared with tests/test_bridge_ref_cpu.py, which pins
the reference (tests/bridge_ref.py) on exactly these inputs and checks what the constructions promise (coverage of the
truncation lengths, which rows overflow, the size conditions) before any GPU is involved.

Every id handed to a kernel lies inside the vocabulary and every substituted column inside its row; the overflow cases use the
kernel's defined overflow path (a counted row that is not served)."""
import functools
from types import SimpleNamespace as NS

import numpy as np

from conzic_amd import harness, synth
from conzic_amd.bridge import tables_from_tokenizers
from conzic_amd.text import tokenizers_from_vocab
from bridge_ref import BridgeRef

PROMPT = ("image", "of", "the", "picture", "photo")
T0, B0, K0 = 12, 3, 70   # 210 threads: four work-groups of 64, the last one partial, and every wave spans two rows of inp


@functools.lru_cache(maxsize=None)
def vocab(tiny=True):
    sv = harness.cached_vocab(tiny)
    tok = sv.bert_tokens
    V = len(tok)
    bt, ct = tokenizers_from_vocab(sv)
    ids = {t: i for i, t in enumerate(tok)}
    irregular = [i for i in range(sv.regular_lo) if tok[i].isascii() and tok[i].isalpha() and len(tok[i]) >= 2 and tok[i] not in PROMPT]
    sentinel = max(irregular, key=lambda i: (len(tok[i]), tok[i]))   # stands in the substituted cell of inp: never decoded
    irregular.remove(sentinel)
    pieces = [i for i in range(V) if tok[i].startswith("##") and tok[i][2:].isascii() and tok[i][2:].isalpha()]
    rng = np.random.default_rng(4242)
    return NS(sv=sv, tok=tok, V=V, id=ids, tables=tables_from_tokenizers(bt, ct), ref=BridgeRef(tok, sv.clip_vocab, sv.clip_merges),
              irregular=irregular, regular=list(range(sv.regular_lo, sv.regular_hi)), pieces=pieces, sentinel=sentinel,
              numbers=[i for i in range(V) if tok[i].isdigit() and len(tok[i]) >= 2],
              special=[ids[t] for t in ("[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]")],
              lexicon=synth.make_lexicon(V), tags=synth.make_pos_tags(V),
              lex_pos=rng.uniform(-1.0, 1.0, size=(V, 5)).astype(np.float32), lex_cls=rng.integers(0, 5, size=V).astype(np.uint8))


def class_ids(vc, b=0):
    """one id list holding every class of token the bridge treats differently (60 ids; b rotates the words chosen)"""
    t = vc.id
    rot = lambda lst, n: [lst[(7 * b + j) % len(lst)] for j in range(n)]
    four = [i for i in vc.pieces if len(vc.tok[i]) == 6]
    out = list(vc.special)                                                                  # id 0 = [PAD] first
    out += [t["[unused0]"], t["[unused2]"]]
    out += [t[x] for x in ("##s", "##ed", "##ing", "##ly", "##er")] + rot(four, 1)          # '##' + letters
    out += [t[x] for x in ("##'", "##.", "##2", "##é")]
    out += [t[x] for x in ("'s", "n't", "'m", "'ve", "'re", "...", "--")]
    out += [t[x] for x in "'.,!?-#\""]
    out += [t["0"], t["7"]] + rot(vc.numbers, 3)
    out += [t[x] for x in ("é", "ß", "α", "中", "ﬁ", "あ")]
    out += rot(vc.irregular, 6) + rot(vc.regular, 6) + [t[x] for x in PROMPT]
    assert len(out) == 60 and vc.sentinel not in out
    return out


def candidates(vc, row, gen, K, rng, b=0, n_tok=None):
    """K candidate ids for one row: every class, five ids the row already holds (repeats > 0), then seeded random ids"""
    n_tok = len(row) if n_tok is None else n_tok
    held = [int(row[c]) for c in range(1, n_tok) if c != gen and int(row[c]) != vc.sentinel]
    out = class_ids(vc, b) + [held[j % len(held)] for j in range(5)]
    while len(out) < K:
        i = int(rng.integers(0, vc.V))
        if i != vc.sentinel:
            out.append(i)
    return out[:K]


def body_token(vc, rng):
    u = rng.random()
    if u < 0.40:
        return int(rng.choice(vc.regular))
    if u < 0.55:
        return int(rng.choice(vc.irregular))
    if u < 0.75:
        return int(rng.choice(vc.pieces))
    if u < 0.90:
        return vc.id[str(rng.choice(["'s", "n't", ",", ".", "'", "-", "...", "##'", "##.", "##2", "7", "0", "é", "中"]))]
    return vc.id[str(rng.choice(PROMPT))]


def base_rows(vc, B, T, gens, rng, row_len=None):
    """[CLS] body [SEP] rows whose substituted cell holds the sentinel word; with row_len the [SEP] sits at row_len - 1 and the
    tail behind it is filled by the caller"""
    inp = np.zeros((B, T), np.int32)
    for b in range(B):
        n = T if row_len is None else int(row_len[b])
        inp[b] = [body_token(vc, rng) for _ in range(T)]
        inp[b, 0] = vc.id["[CLS]"]
        inp[b, n - 1] = vc.id["[SEP]"]
        assert 1 <= gens[b] < n - 1
        inp[b, gens[b]] = vc.sentinel
    return inp


def with_cands(vc, inp, gens, K, rng, row_len=None, **kw):
    B = inp.shape[0]
    cand = np.array([candidates(vc, inp[b], gens[b], K, rng, b, None if row_len is None else int(row_len[b])) for b in range(B)], np.int32)
    return NS(inp=inp, gen=gens, cand=cand, row_len=row_len, **kw)


# ---- 1. the scalar form ---------------------------------------------------------------------------------------------------------
def scalar_case(vc, gen_idx, T=T0, B=B0, K=K0):
    rng = np.random.default_rng(100 + gen_idx)
    gens = [gen_idx] * B
    return with_cands(vc, base_rows(vc, B, T, gens, rng), gens, K, rng)


# ---- 2. the tabulated-piece path next to glued pieces and contraction splits ---------------------------------------------------------
def fast_path_case(vc):
    """A letters-only tabulated piece X directly behind the substituted cell (row 0: a regular word; row 1: '##ing', glued to
    whatever stands there) and directly in front of it (row 2); fixed neighbours of each kind stand elsewhere in the rows."""
    t, R, S = vc.id, vc.regular, vc.sentinel
    rows = [["[CLS]", "image", S, R[0], "of", "'s", R[1], "##ed", ",", "7", R[2], "[SEP]"],
            ["[CLS]", "the", R[3], S, "##ing", "of", "'", R[4], "##s", "##'", R[5], "[SEP]"],
            ["[CLS]", R[6], S, "of", vc.irregular[0], "##er", "the", vc.numbers[0], R[7], "##ly", "n't", "[SEP]"]]
    inp = np.array([[t[x] if isinstance(x, str) else x for x in r] for r in rows], np.int32)
    gens = [2, 3, 2]
    for x in (R[0], t["##ing"], R[6]):   # tabulated: all letters and at most 8 CLIP ids standing alone
        piece = vc.tok[x][2:] if vc.tok[x].startswith("##") else vc.tok[x]
        assert piece.isalpha() and len(vc.ref.bpe.bpe_word(piece)) <= 8
    return with_cands(vc, inp, gens, K0, np.random.default_rng(200))


# ---- 3. the rows form ------------------------------------------------------------------------------------------------------------
def fill_tail(vc, c, rng):
    """columns behind row_len: copies of candidate ids, long words and word-start pieces -- a read of the tail changes the ids,
    the repeat count and all three scores"""
    B, T = c.inp.shape
    for b in range(B):
        n = int(c.row_len[b])
        for col in range(n, T):
            pick = (col - n) % 3
            c.inp[b, col] = (c.cand[b, (5 * col + b) % c.cand.shape[1]] if pick == 0 else
                             vc.irregular[(col + b) % len(vc.irregular)] if pick == 1 else vc.regular[(3 * col + b) % len(vc.regular)])
            if c.inp[b, col] == vc.sentinel or c.inp[b, col] in vc.special:
                c.inp[b, col] = vc.regular[col]
    return c


def rows_case(vc, with_len):
    rng = np.random.default_rng(300)
    gens = [2, 9, 4]
    row_len = np.array([4, 12, 7], np.int32)
    c = with_cands(vc, base_rows(vc, B0, T0, gens, rng, row_len), gens, K0, rng, row_len)
    fill_tail(vc, c, rng)
    if not with_len:
        c.row_len = None   # the same buffers read whole: the tail is part of the sentence
    return c


def score_rows_case(vc, B=130, T=T0):
    """the czc_score_rows shape: K = 1, three work-groups, every thread in a row of inp of its own"""
    rng = np.random.default_rng(301)
    row_len = rng.integers(4, T + 1, size=B).astype(np.int32)
    gens = [int(rng.integers(1, n - 1)) for n in row_len]
    inp = base_rows(vc, B, T, gens, rng, row_len)
    cls = class_ids(vc)
    cand = np.array([[cls[b % len(cls)] if b % 3 else int(inp[b, 1 if gens[b] != 1 else 2])] for b in range(B)], np.int32)
    return fill_tail(vc, NS(inp=inp, gen=gens, cand=cand, row_len=row_len), rng)


# ---- 4. the per-row control signal -------------------------------------------------------------------------------------------------
HP_CONTROLS = [(0, 0), (1, 0), (1, 1), (2, 0), (1, 0), (0, 1)]
HP_TEMPLATE = [["DET"], ["ADJ", "NOUN"], ["NOUN"], ["VERB"], "", ["ADV", "X"], "NOUN", ["."]]


def hp_case(vc):
    rng = np.random.default_rng(400)
    gens = [1, 3, 5, 4, 9, 2]
    row_len = np.array([12, 9, 12, 7, 11, 5], np.int32)
    c = with_cands(vc, base_rows(vc, 6, T0, gens, rng, row_len), gens, K0, rng, row_len, controls=HP_CONTROLS, template=HP_TEMPLATE)
    return fill_tail(vc, c, rng)


# ---- 5. POS templates ------------------------------------------------------------------------------------------------------------
POS_TEMPLATES = {
    # 14 entries over rows of about 8 words: the slots behind the last word are padded with the "" tag, which a STRING entry
    # accepts (substring test), a list entry only if it holds ""; [""] in front accepts no real tag
    "long": [["DET"], "NOUN", ["ADJ", "NOUN"], [""], ["VERB"], ["NOUN", "."], "", ["NUM", "X"], ["NOUN"], "VERB", [""], ["NOUN", ""],
             "", []],
    "short": [["NOUN", "VERB", "ADJ"], "DET", ["X", ".", "PRT"]],            # words beyond the third are ignored
    "wild": ["", "", "", "", ""],
    "nothing": [[], ["NOUN", "ADP", "PRON"], []],
}


def pos_case(vc):
    return scalar_case(vc, 5)


# ---- 6. truncation at 75 body tokens ---------------------------------------------------------------------------------------------------
def body_lengths(vc, rows):
    """per candidate row: (untruncated number of body tokens, whether token 75 and token 76 belong to one pre-split chunk)"""
    out = []
    for ids in rows:
        counts = [len(c) for _, c in vc.ref.chunks(ids)]
        n, run, inside = sum(counts), 0, False
        for m in counts:
            inside |= run < 75 < run + m
            run += m
        out.append((n, inside))
    return out


def truncation_case(vc, T, n_rows=4, K=8, stream=48):
    """rows of a seeded stream with K seeded substitutions each; kept are the first rows that bring a body length not seen yet
    among 73 (clip_len 75), 74, 75 (77, nothing cut), more (cut), and cut inside a multi-token word"""
    rng = np.random.default_rng(600 + T)
    kept, seen = [], set()
    for _ in range(stream):
        n_body = int(rng.integers(T // 3, T - 1))   # the rest of the row is [PAD]
        row = np.full(T, vc.id["[PAD]"], np.int32)
        row[0] = vc.id["[CLS]"]
        body = rng.integers(0, vc.V, size=n_body)
        body[body == vc.sentinel] = vc.regular[0]
        row[1:1 + n_body] = body
        row[1 + n_body] = vc.id["[SEP]"]
        gen = int(rng.integers(1, 1 + n_body))
        row[gen] = vc.sentinel
        cand = rng.integers(0, vc.V, size=K).astype(np.int32)
        cand[cand == vc.sentinel] = vc.regular[1]
        tags = set()
        for n, inside in body_lengths(vc, BridgeRef.spliced(row[None, :], gen, cand[None, :])):
            tags.add("cut" if n > 75 else n)
            if n > 75 and inside:
                tags.add("cut inside a word")
        new = (tags & {73, 74, 75, "cut", "cut inside a word"}) - seen
        if new and len(kept) < n_rows:
            kept.append((row, gen, cand))
            seen |= new
    return NS(inp=np.stack([k[0] for k in kept]), gen=[k[1] for k in kept], cand=np.stack([k[2] for k in kept]), row_len=None, seen=seen)


def full_vocab_case(vc, T=40, B=4, K=K0):
    rng = np.random.default_rng(650)
    gens = [int(g) for g in rng.integers(1, T - 1, size=B)]
    inp = rng.integers(0, vc.V, size=(B, T)).astype(np.int32)
    inp[inp == vc.sentinel] = vc.regular[0]
    inp[:, 0], inp[:, -1] = vc.id["[CLS]"], vc.id["[SEP]"]
    for b in range(B):
        inp[b, gens[b]] = vc.sentinel
    return with_cands(vc, inp, gens, K, rng)


# ---- 7. overflow ------------------------------------------------------------------------------------------------------------------
def text_overflow_case(vc, T=64):
    """Rows of long words whose text, the candidate aside, takes 503 bytes: a one-letter candidate gives 505 (served: the kernel
    keeps two bytes in hand for a leading '##', so 510 is the most it takes), a nine-letter one 513 > 512 (counted, not served).
    Row 0 gets four long candidates, row 1 one."""
    nine = [i for i in vc.irregular if len(vc.tok[i]) == 9]
    assert len(nine) >= 4 and len(vc.tok[vc.sentinel]) == 9
    inp = np.full((2, T), vc.id["[PAD]"], np.int32)
    gens = [20, 45]
    three = next(i for i in vc.irregular + vc.regular if len(vc.tok[i]) == 3)
    for b in range(2):
        words = [nine[(j + b) % len(nine)] for j in range(50)] + [three]    # 50 * 10 + 4 bytes, less the first word's space
        row = [vc.id["[CLS]"]] + words
        row.insert(gens[b], vc.sentinel)
        assert sum(len(vc.tok[w]) + 1 for w in words) - 1 == 503 and len(row) < T
        inp[b, :len(row)] = row
        inp[b, -1] = vc.id["[SEP]"]
    t = vc.id
    short = [t["a"], t[","], t["##s"], t["[PAD]"], t["0"], t["é"], t["'"], t["[MASK]"]]
    cand = np.array([short[:2] + nine[:2] + short[2:4] + nine[2:4] + short[4:], short[:5] + nine[1:2] + short[5:] + short[:3]], np.int32)
    return NS(inp=inp, gen=gens, cand=cand, row_len=None, n_over=5)


def chunk_overflow_case(vc, T=40):
    """One word of glued '##' letter pieces around the substituted cell: 30 bytes in front of it, 32 behind.  A '##' candidate of
    two letters makes a chunk of exactly 64 bytes (served), longer ones overflow the chunk buffer; a candidate that starts a
    word, or is no letter, splits the chunk; a special candidate drops out and leaves 62."""
    four = [i for i in vc.pieces if len(vc.tok[i]) == 6]
    word = next(i for i in vc.regular if len(vc.tok[i]) == 6)
    left, right = four[:6], four[6:14]
    assert len(right) == 8
    row = [vc.id["[CLS]"], vc.id["the"], word] + left + [vc.sentinel] + right + [vc.id["of"], vc.regular[5]]
    gen = 3 + len(left)
    row += [vc.id["[PAD]"]] * (T - 1 - len(row)) + [vc.id["[SEP]"]]
    inp = np.array([row], np.int32)
    cand = np.array([candidates(vc, inp[0], gen, K0, np.random.default_rng(700))], np.int32)
    n_over = 0
    for c in cand[0].tolist():
        s = vc.tok[c]
        glued = 0 if c in vc.special else len(s[2:].encode()) if s.startswith("##") and s[2:].isalpha() else None
        n_over += glued is not None and 30 + glued + 32 > 64
    return NS(inp=inp, gen=[gen], cand=cand, row_len=None, n_over=int(n_over))
