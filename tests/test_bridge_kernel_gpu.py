"""-m gpu: bridge_kernel (conzic_amd/csrc/bridge.hip) in the work it does in production -- candidate substitution, the repeat count,
the three control scores, the per-row column / length form and the per-row control form -- launched alone through
czc_test_bridge_cand and compared WORD FOR WORD, whole buffers and guard words, with the string-level reference
tests/bridge_ref.py (oracle/text.py's decode -> normalise -> pre-split -> BPE; pinned on these very inputs by
tests/test_bridge_ref_cpu.py).  Inputs: tests/bridge_cases.py.

Every launch runs twice, with the per-token piece table (the product's fast path) and with "bridge_no_table" (every chunk
through the merge loop): both must equal the reference.

Conditions, not tolerances: a case that is not about overflow asserts from the reference that every row's text takes at most 500
bytes and every chunk at most 64 (the kernel's buffers: 512 and 64), and no row is left out of a comparison.  Ids, lengths and
repeat counts are exact.  Lexicon sums are compared bit for bit (the reference adds the same fp32 terms in the same order); a
difference would be reported against an fp64 sum and bounded by n_pieces * 2^-24 * sum|term|.  Observed on the MI355X: no
difference in any case (worst deviation 0).  A POS score must satisfy round(score * n) == matches and lie within one float32 ulp
of matches / n.
"""
import numpy as np
import pytest

import bridge_cases as BC
import kernel_hooks as KH
from conzic_amd import native, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vc():
    return BC.vocab(True)


def launch_both(vc, form, c, **kw):
    """-> [(refused, outputs)] with the piece table and without it"""
    lib = native.load_test()
    out = []
    try:
        for no_table in (0, 1):
            assert lib.czc_test_set_option(b"bridge_no_table", no_table) == 0
            gen = c.gen[0] if form == 0 else c.gen
            out.append(KH.bridge_cand(vc.tables, form, c.inp, gen, c.cand, row_len=c.row_len if form else None, **kw))
    finally:
        lib.czc_test_set_option(b"bridge_no_table", 0)
    return out


def lexicon_sums_equal(vc, got_bits, e, lexicon, lex_pos, lex_cls, negative_of_row):
    """bit for bit; where not, the deviation is held against the fp64 sum of the same terms"""
    bad = np.nonzero(got_bits != e["senti_bits"])[0]
    worst = 0.0
    for r in bad:
        terms = [float(lex_pos[i, int(lex_cls[i])]) for i, st in vc.ref.pieces(e["rows"][r]) if st] if lex_pos is not None else \
            [float(lexicon[i]) for i, _ in vc.ref.pieces(e["rows"][r])]
        exact = (-1.0 if negative_of_row(r) else 1.0) * float(np.sum(np.array(terms, np.float64)))
        dev = abs(float(got_bits[r:r + 1].view(np.float32)[0]) - exact)
        bound = len(terms) * 2.0 ** -24 * float(np.sum(np.abs(terms)))
        print(f"row {r}: sum differs from the reference's fp32 sum, deviation from fp64 {dev:.3e} (bound {bound:.3e})")
        worst = max(worst, dev)
        assert dev <= bound, (r, dev, bound)
    assert bad.size == 0, f"{bad.size} lexicon sums are not bit-identical (worst deviation from fp64 {worst:.3e})"


def check(vc, form, c, e, outs, negative=0, lexicon=None, lex_pos=None, lex_cls=None, template=None, served=None):
    """every output of both launches against the reference `e`; served: mask of the rows that must be served (None: all)"""
    N = e["clip_len"].size
    K = c.cand.shape[1]
    rows = np.arange(N) if served is None else np.nonzero(served)[0]
    if served is None:
        assert e["sizes"][:, 0].max() <= 500 and e["sizes"][:, 1].max() <= 64, e["sizes"].max(axis=0)
    for refused, g in outs:
        assert not refused
        g.assert_guards()
        np.testing.assert_array_equal(g["clip_len"][rows], e["clip_len"][rows])
        np.testing.assert_array_equal(g["clip_ids"][rows], e["clip_ids"][rows])
        np.testing.assert_array_equal(g["repeats"].view(np.uint32)[rows], e["repeats_bits"][rows])
        got = g["senti_raw"].view(np.uint32)
        if template is not None or hasattr(c, "controls"):
            pos_rows = rows[e["pos_matches"][rows] >= 0]
            n = len(template if template is not None else c.template)
            score = got[pos_rows].view(np.float32)
            assert np.array_equal(np.round(score.astype(np.float64) * n).astype(np.int64), e["pos_matches"][pos_rows])
            want = (e["pos_matches"][pos_rows] / n).astype(np.float32)
            assert (np.abs(score - want) <= np.spacing(want)).all()
            rest = rows[e["pos_matches"][rows] < 0]
        else:
            rest = rows
        if rest.size:
            sub = dict(e, senti_bits=e["senti_bits"][rest], rows=[e["rows"][r] for r in rest])
            neg = (lambda r: c.controls[rest[r] // K][1]) if hasattr(c, "controls") else (lambda r: negative)
            lexicon_sums_equal(vc, got[rest], sub, lexicon, lex_pos, lex_cls, neg)
    (_, a), (_, b) = outs   # and therefore each other: with the table and without it
    for name in ("clip_ids", "clip_len", "senti_raw", "repeats"):
        np.testing.assert_array_equal(a[name].view(np.uint32)[rows], b[name].view(np.uint32)[rows])


CONTROL_TABLES = ["lexicon", "lex_pos", "pos", "none"]


def tables_kw(vc, which, template=None):
    if which == "lexicon":
        return dict(lexicon=vc.lexicon), dict(lexicon=vc.lexicon)
    if which == "lex_pos":
        return dict(lex_pos=vc.lex_pos, lex_cls=vc.lex_cls), dict(lex_pos=vc.lex_pos, lex_cls=vc.lex_cls)
    if which == "pos":
        return dict(tag_of_token=vc.tags, masks=synth.pos_template_masks(template)), dict(tag_of_token=vc.tags, template=template)
    return {}, {}


# ---- 1. ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("negative", [0, 1])
@pytest.mark.parametrize("which", CONTROL_TABLES)
@pytest.mark.parametrize("gen_idx", [1, 5, BC.T0 - 2])
def test_scalar_form(vc, gen_idx, which, negative):
    """launch_bridge with candidates.  At gen_idx = 1, behind [CLS], a '##' candidate is the first piece and keeps its '##'.  The
    cell of inp at gen_idx holds a long word found nowhere else: it must neither show in an output nor be counted."""
    c = BC.scalar_case(vc, gen_idx)
    kw_k, kw_r = tables_kw(vc, which, BC.HP_TEMPLATE)
    e = vc.ref.expected(c.inp, gen_idx, c.cand, negative=negative, **kw_r)
    outs = launch_both(vc, 0, c, negative=negative, **kw_k)
    check(vc, 0, c, e, outs, negative=negative, template=kw_r.get("template"), **{k: v for k, v in kw_r.items() if k.startswith("lex")})
    for _, g in outs:
        assert int(g["overflow"][0]) == 0
    if gen_idx == 1:   # the construction: some candidate is a leading '##' piece, and the reference keeps its prefix
        k = c.cand[0].tolist().index(vc.id["##ing"])
        assert vc.ref.text(e["rows"][k]).startswith("##ing")
    assert all(vc.sentinel not in r for r in e["rows"])   # the reference never sees the masked cell: an output that equals it holds none of it


# ---- 2. ------------------------------------------------------------------------------------------------------------------------
def test_fast_path_next_to_glue_and_contractions(vc):
    """A tabulated all-letter piece right behind ', ##', 's, a digit or a '##' letter piece, and right in front of a '##' piece: it
    may take its ids from the table only when it is a pre-split chunk of its own."""
    c = BC.fast_path_case(vc)
    e = vc.ref.expected(c.inp, c.gen, c.cand, lexicon=vc.lexicon)
    outs = launch_both(vc, 1, c, lexicon=vc.lexicon)
    check(vc, 1, c, e, outs, lexicon=vc.lexicon)


# ---- 3. ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", CONTROL_TABLES)
@pytest.mark.parametrize("with_len", [False, True])
def test_rows_form(vc, with_len, which):
    """launch_bridge_rows: the column per row; with row_len = [4, 12, 7] the tail behind a row's length holds copies of candidate
    ids, long words and scored word starts, so a read of it changes ids, repeat counts and all three scores."""
    c = BC.rows_case(vc, with_len)
    kw_k, kw_r = tables_kw(vc, which, BC.HP_TEMPLATE)
    e = vc.ref.expected(c.inp, c.gen, c.cand, c.row_len, **kw_r)
    check(vc, 1, c, e, launch_both(vc, 1, c, **kw_k), template=kw_r.get("template"), **{k: v for k, v in kw_r.items() if k.startswith("lex")})
    if with_len:   # the tail matters: the same buffers read whole give other ids, counts and scores in every row of inp
        whole = vc.ref.expected(c.inp, c.gen, c.cand, None, **kw_r)
        K = c.cand.shape[1]
        for b in (0, 2):
            sl = slice(b * K, (b + 1) * K)
            assert (whole["clip_len"][sl] != e["clip_len"][sl]).all() and (whole["repeats_bits"][sl] != e["repeats_bits"][sl]).any()
            assert which == "none" or (whole["senti_bits"][sl] != e["senti_bits"][sl]).any()


@pytest.mark.parametrize("which", ["lexicon", "pos"])
def test_rows_form_one_candidate_per_row(vc, which):
    """B = 130, K = 1: the shape czc_score_rows launches -- three work-groups, every thread with a column and a length of its own"""
    c = BC.score_rows_case(vc)
    assert c.inp.shape[0] == 130 and c.cand.shape[1] == 1 and len(set(c.gen)) > 5 and len(set(c.row_len.tolist())) > 5
    kw_k, kw_r = tables_kw(vc, which, BC.HP_TEMPLATE)
    e = vc.ref.expected(c.inp, c.gen, c.cand, c.row_len, **kw_r)
    check(vc, 1, c, e, launch_both(vc, 1, c, **kw_k), template=kw_r.get("template"), **{k: v for k, v in kw_r.items() if k.startswith("lex")})


# ---- 4. ------------------------------------------------------------------------------------------------------------------------
def hyper_rows(controls):
    return [native.Hyper(0.02, 2.0, 5.0, 0.1, ctl, neg) for ctl, neg in controls]


@pytest.mark.parametrize("which", ["lexicon", "lex_pos"])
def test_hp_form(vc, which):
    """launch_bridge_rows_hp with controls [0, 1, 1 (negative), 2, 1, 0] and row lengths: the launch carries every table, a row
    scores by its own signal, and a control == 0 row leaves the pre-fill pattern in senti_raw and repeats."""
    c = BC.hp_case(vc)
    kw_k, kw_r = tables_kw(vc, which)
    e = vc.ref.expected(c.inp, c.gen, c.cand, c.row_len, tag_of_token=vc.tags, template=c.template, controls=c.controls, **kw_r)
    outs = launch_both(vc, 2, c, tag_of_token=vc.tags, masks=synth.pos_template_masks(c.template), hyper=hyper_rows(c.controls), **kw_k)
    check(vc, 2, c, e, outs, **kw_r)
    K = c.cand.shape[1]
    for _, g in outs:
        for b, (ctl, _) in enumerate(c.controls):
            un_s, un_r = KH.untouched(g["senti_raw"][b * K:(b + 1) * K]), KH.untouched(g["repeats"][b * K:(b + 1) * K])
            assert un_s.all() and un_r.all() if ctl == 0 else not un_s.any() and not un_r.any()


@pytest.mark.parametrize("missing", ["hp_rows", "cand", "gen_rows"])
def test_hp_form_refuses_missing_arguments(vc, missing):
    c = BC.hp_case(vc)
    kw = dict(lexicon=vc.lexicon, tag_of_token=vc.tags, masks=synth.pos_template_masks(c.template),
              hyper=None if missing == "hp_rows" else hyper_rows(c.controls))
    refused, g = KH.bridge_cand(vc.tables, 2, c.inp, None if missing == "gen_rows" else c.gen, None if missing == "cand" else c.cand,
                                row_len=c.row_len, K=c.cand.shape[1], **kw)
    assert refused
    g.assert_guards()
    for name in ("clip_ids", "clip_len", "senti_raw", "repeats"):
        assert KH.untouched(g[name]).all(), name
    assert int(g["overflow"][0]) == 0


# ---- 5. ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BC.POS_TEMPLATES))
def test_pos_template_shapes(vc, name):
    """a 14-entry template over rows of about 8 words (string and list entries in the padded slots, [""] in front of the last
    word), a 3-entry one (later words ignored), all wildcards, entries that accept nothing"""
    c = BC.pos_case(vc)
    template = BC.POS_TEMPLATES[name]
    kw_k, kw_r = tables_kw(vc, "pos", template)
    e = vc.ref.expected(c.inp, c.gen[0], c.cand, **kw_r)
    n_words = [sum(st for _, st in vc.ref.pieces(r)) for r in e["rows"]]
    assert 6 <= min(n_words) and max(n_words) <= 10 and len(set(e["pos_matches"].tolist())) > (1 if name != "wild" else 0)
    check(vc, 0, c, e, launch_both(vc, 0, c, **kw_k), template=template)


# ---- 6. ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [64, 40])
def test_truncation_at_75_body_tokens(vc, T):
    """rows whose reference lengths are 75, 76, 77 with nothing cut, and cut -- at least once inside a multi-token word"""
    c = BC.truncation_case(vc, T)
    e = vc.ref.expected(c.inp, c.gen, c.cand, lexicon=vc.lexicon)
    lengths = BC.body_lengths(vc, e["rows"])
    assert {73, 74, 75} <= {n for n, _ in lengths} and any(n > 75 and inside for n, inside in lengths)
    assert {75, 76, 77} <= set(e["clip_len"].tolist())
    check(vc, 1, c, e, launch_both(vc, 1, c, lexicon=vc.lexicon), lexicon=vc.lexicon)


def test_full_vocabulary():
    vc = BC.vocab(False)
    c = BC.full_vocab_case(vc)
    assert vc.V == 30522 and c.inp.shape == (4, 40) and c.cand.shape == (4, 70)
    e = vc.ref.expected(c.inp, c.gen, c.cand, lex_pos=vc.lex_pos, lex_cls=vc.lex_cls)
    check(vc, 1, c, e, launch_both(vc, 1, c, lex_pos=vc.lex_pos, lex_cls=vc.lex_cls), lex_pos=vc.lex_pos, lex_cls=vc.lex_cls)


# ---- 7. ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["text", "chunk"])
def test_overflow_is_counted_per_row_and_the_others_are_served(vc, case):
    """One launch in which only some candidate rows take the overflow path: a text past 512 bytes (the rows beside them take
    503..506), or one chunk of glued '##' letter pieces past 64 bytes (the rows beside them include chunks of exactly 64).  The
    count is the number of such rows; every other row equals the reference."""
    c = BC.text_overflow_case(vc) if case == "text" else BC.chunk_overflow_case(vc)
    e = vc.ref.expected(c.inp, c.gen, c.cand, lexicon=vc.lexicon)
    over = vc.ref.overflows(e["sizes"])
    assert over.sum() == c.n_over and 0 < c.n_over < over.size
    assert (e["sizes"][~over, 0] <= 510).all() and (e["sizes"][~over, 1] <= 64).all()
    outs = launch_both(vc, 1, c, lexicon=vc.lexicon)
    for _, g in outs:
        assert int(g["overflow"][0]) == c.n_over
    check(vc, 1, c, e, outs, lexicon=vc.lexicon, served=~over)
