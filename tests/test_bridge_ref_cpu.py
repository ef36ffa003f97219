"""CPU: pins the string-level bridge reference (tests/bridge_ref.py) before tests/test_bridge_kernel_gpu.py holds the kernel
against it -- (a) on the HF golden, (b) on the GPU tests' own seeded inputs (tests/bridge_cases.py) against the three other
statements of the same arithmetic the repository has: the table-level emulator (tests/bridge_emulator.py), oracle/step.py and the
reference's torch expression for the repeat count, (c) the size conditions those inputs must meet for the kernel's fixed buffers,
and what the constructions promise (truncation lengths, which rows overflow)."""
import json
import os

import numpy as np
import pytest
import torch

import bridge_cases as BC
from bridge_emulator import emulate_row
from bridge_ref import CLIP_LEN, UNWRITTEN
from conzic_amd import synth
from goldutil import GOLD
from oracle import step as S


def f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


@pytest.mark.parametrize("label", ["tiny", "full"])
def test_reference_returns_the_hf_ids_on_verbatim_rows(label):
    g = json.load(open(os.path.join(GOLD, "text_bridge.json")))[label]
    vc = BC.vocab(label == "tiny")
    for ids, s, c in zip(g["rows"], g["strings"], g["clip_ids"]):
        row, n = vc.ref.clip_row(ids)
        assert n == len(c) and row[:n] == c and row[n:] == [vc.ref.bpe.eos_id] * (CLIP_LEN - n)
        assert vc.ref.text(ids) == vc.ref.bpe.normalize(s)
    e = vc.ref.expected(np.array([r for r in g["rows"] if len(r) == len(g["rows"][0])], np.int32), 0, None)
    assert e["clip_ids"][0, :e["clip_len"][0]].tolist() == g["clip_ids"][0]


def all_cases(vc):
    yield from ((f"scalar gen {g}", BC.scalar_case(vc, g)) for g in (1, 5, BC.T0 - 2))
    yield "fast path", BC.fast_path_case(vc)
    yield "rows", BC.rows_case(vc, False)
    yield "rows with lengths", BC.rows_case(vc, True)
    yield "score rows", BC.score_rows_case(vc)
    yield "hp", BC.hp_case(vc)
    yield "truncation 64", BC.truncation_case(vc, 64)
    yield "truncation 40", BC.truncation_case(vc, 40)


def oracle_for(vc, **kw):
    return S.Oracle({}, None, {}, None, vc.tok, vc.ref.bpe, **kw)


def check_against_the_other_statements(vc, name, c):
    ref = vc.ref
    e_lex = ref.expected(c.inp, c.gen, c.cand, c.row_len, lexicon=vc.lexicon)
    e_neg = ref.expected(c.inp, c.gen, c.cand, c.row_len, lex_pos=vc.lex_pos, lex_cls=vc.lex_cls, negative=1)
    template = BC.POS_TEMPLATES["long"]
    e_pos = ref.expected(c.inp, c.gen, c.cand, c.row_len, tag_of_token=vc.tags, template=template)
    rows = e_lex["rows"]
    # (c) what the kernel's fixed buffers hold with room to spare
    assert e_lex["sizes"][:, 0].max() <= 500 and e_lex["sizes"][:, 1].max() <= 64, (name, e_lex["sizes"].max(0))
    K = c.cand.shape[1]
    for r, ids in enumerate(rows):
        b, k = divmod(r, K)
        assert vc.sentinel not in ids and len(ids) == (c.inp.shape[1] if c.row_len is None else c.row_len[b])
        # the table-level emulation of the kernel's algorithm, on the device tables
        got = emulate_row(vc.tables, ids)
        assert got == e_lex["clip_ids"][r, :e_lex["clip_len"][r]].tolist(), (name, r)
        assert (e_lex["clip_ids"][r, e_lex["clip_len"][r]:] == vc.tables.eos_id).all()
    # oracle/step.py on the spliced rows (they have one length per row of inp: call it row by row)
    o_lex, o_lp, o_pos = oracle_for(vc, lexicon=vc.lexicon), oracle_for(vc, lexicon_pos=(vc.lex_pos, vc.lex_cls)), oracle_for(vc, pos_tags=vc.tags)
    for r, ids in enumerate(rows):
        t = torch.tensor([ids], dtype=torch.int64)
        terms = [float(vc.lexicon[i]) for i, _ in ref.pieces(ids)]
        bound = len(terms) * 2.0 ** -24 * sum(abs(x) for x in terms)    # two fp32 summation orders of the same terms
        assert abs(float(S.senti_scores(o_lex, t, "positive")[0]) - float(f32(e_lex["senti_bits"])[r])) <= 2 * bound
        assert float(S.senti_scores(o_lp, t, "negative")[0]) == float(f32(e_neg["senti_bits"])[r])       # the same order: exact
        assert np.float32(S.pos_scores(o_pos, t, template)[0].item()) == f32(e_pos["senti_bits"])[r]
        assert round(float(f32(e_pos["senti_bits"])[r]) * len(template)) == e_pos["pos_matches"][r]
    # control_gen_utils.py:53 on the rows as tensors (rows of one length only)
    if c.row_len is None:
        B, T = c.inp.shape
        topk_inp = torch.from_numpy(c.inp.astype(np.int64)).unsqueeze(1).repeat(1, K, 1)
        idxs_ = torch.from_numpy(c.cand.astype(np.int64))
        for b in range(B):
            topk_inp[b, :, c.gen[b]] = idxs_[b]
        repeats = ((idxs_[:, :, None] == topk_inp).float().sum(2) - 1)
        assert np.array_equal(repeats.reshape(-1).numpy(), f32(e_lex["repeats_bits"]))
    return e_lex


def test_reference_on_the_gpu_tests_inputs_equals_emulator_and_oracle():
    vc = BC.vocab(True)
    for name, c in all_cases(vc):
        e = check_against_the_other_statements(vc, name, c)
        rep = f32(e["repeats_bits"]).reshape(c.cand.shape)
        if c.cand.shape[1] == BC.K0:   # the candidate set: at least five repeats per row, [PAD] first, every class present
            assert ((rep > 0).sum(axis=1) >= 5).all(), name
            assert set(BC.class_ids(vc, 0)[:5]) <= set(c.cand[0].tolist()) and c.cand[0, 0] == 0


def test_full_vocabulary_case():
    vc = BC.vocab(False)
    c = BC.full_vocab_case(vc)
    assert c.inp.shape == (4, 40) and c.cand.shape == (4, 70) and vc.V == 30522
    check_against_the_other_statements(vc, "full", c)


def test_hp_case_leaves_control_0_rows_unwritten():
    vc = BC.vocab(True)
    c = BC.hp_case(vc)
    e = vc.ref.expected(c.inp, c.gen, c.cand, c.row_len, lexicon=vc.lexicon, tag_of_token=vc.tags, template=c.template, controls=c.controls)
    K = c.cand.shape[1]
    for b, (ctl, neg) in enumerate(c.controls):
        sl = slice(b * K, (b + 1) * K)
        if ctl == 0:
            assert (e["senti_bits"][sl] == UNWRITTEN).all() and (e["repeats_bits"][sl] == UNWRITTEN).all()
        else:
            one = vc.ref.expected(c.inp[b:b + 1], c.gen[b:b + 1], c.cand[b:b + 1], c.row_len[b:b + 1], lexicon=None if ctl == 2 else vc.lexicon,
                                  tag_of_token=vc.tags if ctl == 2 else None, template=c.template, negative=neg)
            assert np.array_equal(one["senti_bits"], e["senti_bits"][sl]) and (e["senti_bits"][sl] != UNWRITTEN).all()
            assert (e["pos_matches"][sl] >= 0).all() == (ctl == 2)
    # the rows under different signals differ in what they score: using row 0's control for every row cannot pass
    assert len({e["senti_bits"][b * K + 20] for b in range(6)}) >= 4


def kernel_rule(masks, tags):
    """the mask arithmetic of bridge_kernel on a list of word tags: what synth.pos_template_masks must encode"""
    ok = 0
    for w, m in enumerate(masks.tolist()):
        if w < len(tags):
            ok += m == 0xFFFF or (m >> tags[w]) & 1
        else:
            ok += (m & 0x8000) != 0
    return ok


@pytest.mark.parametrize("name", sorted(BC.POS_TEMPLATES))
def test_template_masks_encode_the_python_template(name):
    """synth.pos_template_masks + the kernel's rule == `in` on the template as lists and strings, for every number of words around
    the template's length.  ([""] is a list like any other: it accepts the padding tag and no real one.)"""
    vc = BC.vocab(True)
    template = BC.POS_TEMPLATES[name]
    masks = synth.pos_template_masks(template)
    rng = np.random.default_rng(5)
    words = [i for i in vc.regular[:200]]
    for n in range(0, len(template) + 3):
        for _ in range(6):
            ids = [int(i) for i in rng.choice(words, size=n)]
            tags = [int(vc.tags[i]) for i in ids]
            assert kernel_rule(masks, tags) == vc.ref.pos_matches(ids, vc.tags, template), (name, n)


def test_truncation_cases_cover_the_lengths_around_the_cut():
    vc = BC.vocab(True)
    seen = set()
    for T in (64, 40):
        c = BC.truncation_case(vc, T)
        assert c.cand.shape[1] == 8 and c.inp.shape[1] == T
        e = vc.ref.expected(c.inp, c.gen, c.cand)
        for (n, inside), ln, ids in zip(BC.body_lengths(vc, e["rows"]), e["clip_len"], e["clip_ids"]):
            assert ln == min(n, 75) + 2
            seen.add("cut" if n > 75 else n)
            if n > 75 and inside:
                seen.add("cut inside a word")
                assert ids[75] != vc.tables.eos_id and ids[76] == vc.tables.eos_id
    assert {73, 74, 75, "cut", "cut inside a word"} <= seen, seen


def test_overflow_cases_overflow_where_they_say():
    vc = BC.vocab(True)
    c = BC.text_overflow_case(vc)
    e = vc.ref.expected(c.inp, c.gen, c.cand)
    over = vc.ref.overflows(e["sizes"])
    assert over.sum() == c.n_over == 5 and over.reshape(c.cand.shape).sum(axis=1).tolist() == [4, 1]
    # served rows stay inside what the kernel takes (it keeps two bytes in hand), counted ones are past the buffer
    assert (e["sizes"][~over, 0] <= 510).all() and (e["sizes"][~over, 0] >= 503).all() and (e["sizes"][over, 0] > 512).all()
    assert e["sizes"][:, 1].max() <= 64
    c = BC.chunk_overflow_case(vc)
    e = vc.ref.expected(c.inp, c.gen, c.cand)
    over = vc.ref.overflows(e["sizes"])
    assert over.sum() == c.n_over and 0 < c.n_over < c.cand.size
    assert e["sizes"][:, 0].max() <= 500 and (e["sizes"][~over, 1] == 64).any() and (e["sizes"][over, 1] == 65).any()
    for r in np.nonzero(~over)[0]:
        assert emulate_row(vc.tables, e["rows"][r]) == e["clip_ids"][r, :e["clip_len"][r]].tolist()


# ---- the inputs tell wrong kernels from the right one: each family below changes the expected output of at least one GPU test -------
def test_inputs_separate_the_wrong_kernels_this_suite_is_meant_to_catch():
    vc = BC.vocab(True)
    ref = vc.ref
    ids_of = lambda rows: [ref.clip_row(r)[0] for r in rows]
    # reading the substituted cell of inp (the [MASK] column in production) instead of the candidate: every row changes
    c = BC.scalar_case(vc, 5)
    e = ref.expected(c.inp, 5, c.cand, lexicon=vc.lexicon)
    stale = [c.inp[b].tolist() for b in range(c.inp.shape[0]) for _ in range(c.cand.shape[1])]
    assert all(a != b.tolist() for a, b in zip(ids_of(stale), e["clip_ids"]))
    # reading past row_len: ids, repeat counts and every score change (rows 0 and 2 of the rows case have a tail)
    c = BC.rows_case(vc, True)
    for kw in (dict(lexicon=vc.lexicon), dict(lex_pos=vc.lex_pos, lex_cls=vc.lex_cls), dict(tag_of_token=vc.tags, template=BC.HP_TEMPLATE)):
        e, whole = ref.expected(c.inp, c.gen, c.cand, c.row_len, **kw), ref.expected(c.inp, c.gen, c.cand, None, **kw)
        for b in (0, 2):
            sl = slice(b * BC.K0, (b + 1) * BC.K0)
            assert (e["clip_len"][sl] != whole["clip_len"][sl]).all() and (e["repeats_bits"][sl] != whole["repeats_bits"][sl]).any()
            assert (e["senti_bits"][sl] != whole["senti_bits"][sl]).any()
    # row 0's control for every row: test_hp_case_leaves_control_0_rows_unwritten (rows 1..4 would stay unwritten)
    # skipping the `first` rule: a leading '##' candidate (gen_idx = 1) loses its prefix, its word start and its score
    c = BC.scalar_case(vc, 1)
    e = ref.expected(c.inp, 1, c.cand, lex_pos=vc.lex_pos, lex_cls=vc.lex_cls)
    lead = [r for r, ids in enumerate(e["rows"]) if vc.tok[ids[1]].startswith("##")]
    assert len(lead) >= 3 * 10
    for r in lead:
        ids = e["rows"][r]
        assert ref.text(ids).startswith("##")    # decode_chain leaves piece 0 untouched
        no_first = np.float32(0.0)               # the lex_pos sum with word starts = pieces without '##' only
        for i, _ in ref.pieces(ids):
            if not vc.tok[i].startswith("##"):
                no_first = np.float32(no_first + vc.lex_pos[i, int(vc.lex_cls[i])])
        assert np.array([no_first], np.float32).view(np.uint32)[0] != e["senti_bits"][r]
    # the table path for a glued piece: '##ing' glued to a word is one chunk whose BPE is not the word's ids followed by the piece's
    c = BC.fast_path_case(vc)
    e = ref.expected(c.inp, c.gen, c.cand)
    ing, wrong = ref.bpe.bpe_word("ing"), 0
    for r in range(BC.K0, 2 * BC.K0):               # row 1: the candidate stands right in front of '##ing'
        ids = e["rows"][r]
        prev = vc.tok[ids[3]]
        if prev.isalpha() and ids[3] not in ref.special:
            glued = ref.bpe.bpe_word(prev + "ing")
            wrong += glued != ref.bpe.bpe_word(prev) + ing
    assert wrong >= 10
    # emitting 76 body tokens: every cut row changes
    for T in (64, 40):
        c = BC.truncation_case(vc, T)
        e = ref.expected(c.inp, c.gen, c.cand)
        cut = [r for r, (n, _) in enumerate(BC.body_lengths(vc, e["rows"])) if n > 75]
        assert cut
        for r in cut:
            body = [t for _, ch in ref.chunks(e["rows"][r]) for t in ch]
            assert body[75] != ref.bpe.eos_id and e["clip_ids"][r, 76] == ref.bpe.eos_id and e["clip_ids"][r, 75] == body[74]
