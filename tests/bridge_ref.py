"""Host reference of the text bridge kernel (conzic_amd/csrc/bridge.hip bridge_kernel) in all its forms: candidate substitution,
per-row columns and lengths, per-row control signals.  TEST INFRASTRUCTURE.

It works from TOKEN STRINGS and the oracle's string path (oracle/text.py: decode with clean-up -> CLIP normaliser -> regex
pre-split -> byte-level BPE), not from the device tables (conzic_amd.bridge.BridgeArrays) and not from the kernel's algorithm:
tests/bridge_emulator.py is a line-by-line copy of the kernel and therefore shares its mistakes; this file shares none of its
code.  tests/test_bridge_ref_cpu.py pins it against the HF golden, the emulator and oracle/step.py.

What a candidate row (b, k) of a launch is: the first row_len[b] (else T) ids of inp[b] with column gen[b] replaced by cand[b, k].
  clip ids  oracle.text.bridge of that row, right-padded with <|endoftext|> to 77; clip_len = its unpadded length
  repeats   occurrences of cand[b, k] in that row minus 1, specials included (control_gen_utils.py:53)
  lexicon   fp32 sum, in token order, of lexicon[id] over the non-special pieces
  lex_pos   the same sum of table[id, cls[id]] over the word-start pieces (the first non-special piece, or one without '##')
  negative  negates the score
  POS       tags of the word-start pieces against the template AS PYTHON LISTS AND STRINGS with `in`, padded with "" / cut to
            len(template), "" = wildcard: oracle/step.py::pos_scores, POS_classifier.py:17-29
A control == 0 row of the per-row hyper-parameter form leaves senti_raw and repeats unwritten.
"""
import numpy as np

from conzic_amd.synth import UNIVERSAL_TAGS
from oracle import text as OT

CLIP_LEN = 77
MAX_BYTES = 512     # the kernel's text buffer per row (CZC_BRIDGE_MAX_BYTES)
MAX_CHUNK = 64      # its longest pre-split chunk in bytes
UNWRITTEN = 0x5A5A5A5A   # what a word the kernel must not write reads back as (tests/kernel_hooks.py SENTINEL)


class _MemoBpe(OT.ClipBpe):
    """oracle.text.ClipBpe with the per-chunk result remembered (the K candidate rows of an image share all but one word)."""

    def __init__(self, vocab, merges):
        super().__init__(vocab, merges)
        self._memo = {}

    def bpe_word(self, chunk):
        got = self._memo.get(chunk)
        if got is None:
            got = self._memo[chunk] = super().bpe_word(chunk)
        return list(got)


class BridgeRef:
    def __init__(self, bert_tokens, clip_vocab, clip_merges):
        self.tok = list(bert_tokens)
        self.bpe = _MemoBpe(clip_vocab, clip_merges)
        self.special = {i for i, t in enumerate(self.tok) if t in OT.BERT_SPECIALS}

    # ---- one row of ids --------------------------------------------------------------------------------------------------------
    def clip_row(self, ids):
        """-> (77 ids, unpadded length)"""
        c = OT.bridge([int(i) for i in ids], self.tok, self.bpe)
        assert 2 <= len(c) <= CLIP_LEN
        return c + [self.bpe.eos_id] * (CLIP_LEN - len(c)), len(c)

    def text(self, ids):
        """the decoded caption as the CLIP tokenizer sees it (normalised)"""
        return self.bpe.normalize(OT.bert_decode([int(i) for i in ids], self.tok, skip_special_tokens=True))

    def chunks(self, ids):
        """[(chunk string, its CLIP ids)] of the whole caption, untruncated"""
        return [(c, self.bpe.bpe_word(c)) for c in OT.clip_presplit(self.text(ids))]

    def sizes(self, ids):
        """(bytes of the decoded text, bytes of its longest pre-split chunk): what the kernel's fixed buffers must hold"""
        txt = self.text(ids)
        return len(txt.encode("utf-8")), max([len(c.encode("utf-8")) for c in OT.clip_presplit(txt)] or [0])

    def pieces(self, ids):
        """[(id, is word start)] of the non-special pieces"""
        out, first = [], True
        for i in ids:
            i = int(i)
            if i in self.special:
                continue
            out.append((i, first or not self.tok[i].startswith("##")))
            first = False
        return out

    def lexicon_score(self, ids, lexicon, negative=False):
        s = np.float32(0.0)
        for i, _ in self.pieces(ids):
            s = np.float32(s + np.float32(lexicon[i]))
        return np.float32(-s) if negative else s

    def lex_pos_score(self, ids, table, cls, negative=False):
        s = np.float32(0.0)
        for i, start in self.pieces(ids):
            if start:
                s = np.float32(s + np.float32(table[i, int(cls[i])]))
        return np.float32(-s) if negative else s

    def pos_matches(self, ids, tag_of_token, template):
        """matched template slots (the score is matches / len(template))"""
        tags = [UNIVERSAL_TAGS[int(tag_of_token[i])] for i, start in self.pieces(ids) if start]
        total = len(template)
        cur = tags + [""] * (total - len(tags)) if len(tags) <= total else tags[:total]
        correct = 0
        for w in range(len(cur)):
            if template[w] == "":
                correct += 1
            elif cur[w] in template[w]:
                correct += 1
        return correct

    # ---- a whole launch --------------------------------------------------------------------------------------------------------
    @staticmethod
    def spliced(inp, gen, cand, row_len=None):
        """[B*K] lists of ids: the candidate rows of a launch (gen: an int or [B]; cand None: the rows verbatim)"""
        inp = np.asarray(inp)
        B, T = inp.shape
        gens = [int(gen)] * B if np.isscalar(gen) else [int(g) for g in gen]
        rows = []
        for b in range(B):
            n = T if row_len is None else int(row_len[b])
            if cand is None:
                rows.append(inp[b, :n].tolist())
                continue
            assert 0 <= gens[b] < n, "the substituted column lies inside the row"
            for c in np.asarray(cand)[b].tolist():
                r = inp[b, :n].tolist()
                r[gens[b]] = int(c)
                rows.append(r)
        return rows

    def expected(self, inp, gen, cand, row_len=None, lexicon=None, lex_pos=None, lex_cls=None, tag_of_token=None, template=None,
                 negative=0, controls=None):
        """What the launch must leave in its outputs.  controls (the hyper-parameter form): [(control, negative)] per row of inp --
        control 1 scores by lex_pos (when given) else lexicon, 2 by the POS template, 0 writes neither score.  Without it the
        launch's one signal is the POS template when tags are given, else lex_pos, else lexicon, else an empty sum.
        -> dict: clip_ids [N, 77], clip_len [N], senti_bits, repeats_bits [N] uint32 (bit patterns), pos_matches [N] (-1 where the
        row has no POS score), sizes [N, 2] (text bytes, longest chunk bytes), rows (the spliced id lists)"""
        rows = self.spliced(inp, gen, cand, row_len)
        N = len(rows)
        K = 1 if cand is None else np.asarray(cand).shape[1]
        flat = None if cand is None else np.asarray(cand).reshape(-1)
        out = dict(clip_ids=np.zeros((N, CLIP_LEN), np.int32), clip_len=np.zeros(N, np.int32), senti_bits=np.zeros(N, np.uint32),
                   repeats_bits=np.zeros(N, np.uint32), pos_matches=np.full(N, -1, np.int64), sizes=np.zeros((N, 2), np.int64), rows=rows)
        for r, ids in enumerate(rows):
            ctl, neg = (None, negative) if controls is None else controls[r // K]
            out["clip_ids"][r], out["clip_len"][r] = self.clip_row(ids)
            out["sizes"][r] = self.sizes(ids)
            rep = np.float32((ids.count(int(flat[r])) if flat is not None else 0) - 1)
            if ctl == 0:
                out["senti_bits"][r] = out["repeats_bits"][r] = UNWRITTEN
                continue
            use_pos = tag_of_token is not None and ctl in (None, 2)
            if use_pos:
                m = self.pos_matches(ids, tag_of_token, template)
                out["pos_matches"][r] = m
                s = np.float32(np.float32(m) / np.float32(len(template)))
            elif ctl == 2:
                raise ValueError("a control == 2 row needs the POS tables")
            elif lex_pos is not None:
                s = self.lex_pos_score(ids, lex_pos, lex_cls, neg)
            elif lexicon is not None:
                s = self.lexicon_score(ids, lexicon, neg)
            else:
                s = np.float32(-0.0) if neg else np.float32(0.0)
            out["senti_bits"][r] = np.array([s], np.float32).view(np.uint32)[0]
            out["repeats_bits"][r] = np.array([rep], np.float32).view(np.uint32)[0]
        return out

    def overflows(self, sizes):
        """rows whose text or longest chunk exceeds the kernel's buffers: its defined overflow path (counted, row not served)"""
        sizes = np.asarray(sizes)
        return (sizes[:, 0] > MAX_BYTES) | (sizes[:, 1] > MAX_CHUNK)
