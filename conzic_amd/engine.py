"""Python handle on one native engine (one GPU): thin, typed calls into libconzic_hip.so.

Everything numeric happens in the shared library; this class only marshals numpy buffers (or
device pointers of torch tensors) across the C ABI of include/conzic_hip.h.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import Dict, Iterable, Optional, Sequence

import numpy as np

from . import native
from .bridge import BridgeArrays
from .native import NativeError  # noqa: F401  (re-export)


def _ptr(a):
    """host numpy array or a device tensor (anything with .data_ptr()) -> void*"""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    raise TypeError(type(a))


def hyper_array(hypers: Sequence[native.Hyper]):
    """A contiguous ctypes array of native.Hyper (czc_hyper [R]) holding copies of `hypers`."""
    hs = list(hypers)
    arr = (native.Hyper * max(len(hs), 1))()
    for i, h in enumerate(hs):
        if not isinstance(h, native.Hyper):
            raise TypeError(f"hypers[{i}] is {type(h).__name__}, not native.Hyper")
        C.memmove(C.byref(arr, i * C.sizeof(native.Hyper)), C.byref(h), C.sizeof(native.Hyper))
    return arr if hs else arr[:0]


def draw_array(draws: Sequence[native.Draw]):
    """A contiguous ctypes array of native.Draw (czc_draw [R]) holding copies of `draws`."""
    ds = list(draws)
    arr = (native.Draw * max(len(ds), 1))()
    for i, d in enumerate(ds):
        if not isinstance(d, native.Draw):
            raise TypeError(f"draws[{i}] is {type(d).__name__}, not native.Draw")
        arr[i].seed, arr[i].tau, arr[i].step0 = d.seed, d.tau, d.step0
    return arr if ds else arr[:0]


_ABSENT = object()   # an argument the method does not have (None is a value: NULL, or zeros for deltas)


def _row_vector(name: str, what: str, x, n: int, unit: str = "rows", dtype=np.int32):
    """contiguous 1-D `dtype` array of n entries from `x` (None passes through); `name`: the method, for the ValueError text"""
    if x is None:
        return None
    v = np.ascontiguousarray(x, dtype=dtype).reshape(-1)
    if v.size != n:
        raise ValueError(f"{name}: {what} has {v.size} entries for {n} {unit}")
    return v


def _rival_table(name: str, rivals, R: int):
    """int32 [R, M] from `rivals` (None passes through)."""
    if rivals is None:
        return None
    rv = np.ascontiguousarray(rivals, dtype=np.int32)
    if rv.ndim != 2 or rv.shape[0] != R or rv.shape[1] < 1:
        raise ValueError(f"{name}: rivals must be [R, M] with R = {R} and M >= 1, got {rv.shape}")
    return rv


def _vocab_sets(name: str, sets, V: int):
    """uint32 [n_sets, W] bitsets from `sets` (one set [W] becomes [1, W]); W = ceil(V / 32), conzic_amd.vocab.pack builds such a table"""
    bits = np.ascontiguousarray(sets, dtype=np.uint32)
    if bits.ndim == 1:
        bits = bits.reshape(1, -1)
    if bits.ndim != 2 or bits.shape[1] != (V + 31) // 32:
        raise ValueError(f"{name}: sets must be uint32 [n_sets, {(V + 31) // 32}] (one bit per id of the {V}-id vocabulary), got {bits.shape}")
    return bits


def make_config(bert_cfg, clip_cfg, special: Dict[str, int], precision: int) -> native.Config:
    c = native.Config()
    if bert_cfg is not None:
        c.bert_vocab, c.bert_hidden, c.bert_layers = bert_cfg.vocab, bert_cfg.hidden, bert_cfg.layers
        c.bert_heads, c.bert_inter, c.bert_max_pos, c.bert_eps = bert_cfg.heads, bert_cfg.inter, bert_cfg.max_pos, bert_cfg.eps
    else:
        c.bert_vocab = c.bert_layers = 0
        c.bert_hidden, c.bert_heads, c.bert_inter, c.bert_max_pos, c.bert_eps = 64, 1, 64, 1, 1e-12
    c.clip_vocab, c.clip_hidden, c.clip_layers, c.clip_heads = clip_cfg.vocab, clip_cfg.hidden, clip_cfg.layers, clip_cfg.heads
    c.clip_inter, c.clip_max_pos, c.clip_proj, c.clip_eps = clip_cfg.inter, clip_cfg.max_pos, clip_cfg.proj, clip_cfg.eps
    c.clip_bos_id, c.clip_eos_id = clip_cfg.bos_id, clip_cfg.eos_id
    c.vis_hidden, c.vis_layers, c.vis_heads, c.vis_inter = clip_cfg.v_hidden, clip_cfg.v_layers, clip_cfg.v_heads, clip_cfg.v_inter
    c.vis_image, c.vis_patch = clip_cfg.v_image, clip_cfg.v_patch
    c.pad_id = special.get("[PAD]", 0)
    c.unk_id = special.get("[UNK]", 0)
    c.cls_id = special.get("[CLS]", 0)
    c.sep_id = special.get("[SEP]", 0)
    c.mask_id = special.get("[MASK]", 0)
    c.dot_id = special.get(".", 0)
    c.precision = precision
    return c


def normalize_state_name(name: str) -> Optional[str]:
    """Checkpoint key -> the name the engine knows, or None for tensors the path never reads.
    `from_pretrained` renames the legacy TF-style `LayerNorm.gamma` / `LayerNorm.beta` of old BERT checkpoints to
    `.weight` / `.bias` on load; a safetensors file read directly still carries the old names.  The pooler and the
    next-sentence head are not on the masked-LM path (HF:bert/modeling_bert.py:939-982); `position_ids` is a
    buffer; the MLM decoder weight is tied to the word embeddings (HF:bert/modeling_bert.py:910-913)."""
    if name.endswith(".gamma"):
        name = name[:-len(".gamma")] + ".weight"
    elif name.endswith(".beta"):
        name = name[:-len(".beta")] + ".bias"
    if name.endswith("position_ids") or name == "cls.predictions.decoder.weight":
        return None
    if name.startswith("bert.pooler.") or name.startswith("cls.seq_relationship."):
        return None
    return name


class Engine:
    def __init__(self, bert_cfg, clip_cfg, special: Dict[str, int], precision: int = native.PREC_BF16, device: int = 0):
        self.lib = native.load()
        self.cfg = make_config(bert_cfg, clip_cfg, special, precision)
        self.bert_cfg, self.clip_cfg = bert_cfg, clip_cfg
        self.precision = precision
        h = C.c_void_p()
        native.check(self.lib.czc_create(C.byref(self.cfg), device, C.byref(h)), None, "czc_create")
        self.h = h
        self._keep = []  # host arrays the engine may still point at
        self._replay = {}    # last call of every per-engine setter: replayed on replicas (they share only the weights)
        self._replicas = []
        self._parent = None

    # ---- lifecycle --------------------------------------------------------------------------
    def close(self):
        g = getattr(self, "_group", None)  # runtime.py caches its EngineGroup here
        if g is not None and g._pool is not None:
            g._pool.shutdown(wait=True)
            g._pool = None
        self._group = None
        for r in getattr(self, "_replicas", []):
            r.close()  # replicas point at this engine's weights: they go first
        self._replicas = []
        if getattr(self, "h", None):
            self.lib.czc_destroy(self.h)
            self.h = None

    def replica(self) -> "Engine":
        """A second engine on the same GPU over the SAME weights (czc_replicate): own stream, workspace, image
        embeddings and tables.  Every setter call made on this engine so far is replayed on it, later ones are
        forwarded.  Closed with (before) its parent."""
        if self._parent is not None:
            parent = self._parent()
            if parent is None or parent.h is None:
                raise NativeError("replica(): the parent engine of this replica was closed (it owns the weights)")
            return parent.replica()
        if self.h is None:
            raise NativeError("replica(): this engine is closed")
        r = object.__new__(Engine)
        r.lib, r.cfg, r.bert_cfg, r.clip_cfg, r.precision = self.lib, self.cfg, self.bert_cfg, self.clip_cfg, self.precision
        import weakref
        r._keep, r._replay, r._replicas, r._parent = [], {}, [], weakref.ref(self)  # no parent <-> replica cycle: both have __del__
        h = C.c_void_p()
        self._ck(self.lib.czc_replicate(self.h, C.byref(h)), "czc_replicate")
        r.h = h
        for name, (fn, args) in list(self._replay.items()):
            getattr(r, fn)(*args)
        self._replicas.append(r)
        return r

    def _record(self, key, fn, *args):
        self._replay[key] = (fn, args)
        for r in self._replicas:
            getattr(r, fn)(*args)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if rc != 0 and getattr(self, "h", None) is None:
            raise NativeError(f"{what}: this engine is closed" + (" (a replica is closed with its parent, which owns the weights)"
                                                                  if self._parent is not None else ""))
        native.check(rc, self.h, what)

    # ---- frozen state -------------------------------------------------------------------------
    def load_state(self, *state_dicts, names: Optional[Iterable[str]] = None):
        """Each state dict maps HF names to fp32 arrays: numpy, or torch tensors (CPU or on this
        GPU -- device tensors are consumed in place, which is the RCCL-broadcast hand-over)."""
        for sd in state_dicts:
            for name, t in sd.items():
                if names is not None and name not in names:
                    continue
                name = normalize_state_name(name)
                if name is None:
                    continue
                if name == "cls.predictions.decoder.bias" and "cls.predictions.bias" in sd:
                    continue
                if hasattr(t, "detach"):
                    t = t.detach()
                    if t.dtype is not __import__("torch").float32:
                        t = t.float()
                    t = t.contiguous()
                    shape = tuple(t.shape)
                    src = t.data_ptr()
                    self._tmp = t
                else:
                    t = np.ascontiguousarray(t, dtype=np.float32)
                    shape = t.shape
                    src = t.ctypes.data
                    self._tmp = t
                sh = (C.c_int64 * max(1, len(shape)))(*shape)
                self._ck(self.lib.czc_load_tensor(self.h, name.encode(), 0, len(shape), sh, src), f"czc_load_tensor({name})")
        self._tmp = None

    def finalize(self):
        self._ck(self.lib.czc_finalize_weights(self.h), "czc_finalize_weights")

    def set_token_mask(self, mask):
        m = np.ascontiguousarray(np.asarray(mask, dtype=np.float32).reshape(-1))
        self._ck(self.lib.czc_set_token_mask(self.h, m.ctypes.data, m.size), "czc_set_token_mask")
        self._record("token_mask", "set_token_mask", m)

    def set_lexicon_pos(self, table, class_of_token):
        """(word-start piece, coarse POS class) keyed sentiment table [V,5] + class per token [V] (None: back to
        the per-token lexicon).  See conzic_amd/sentiment.py."""
        if table is None:
            self._ck(self.lib.czc_set_lexicon_pos(self.h, None, None, 0), "czc_set_lexicon_pos")
            self._record("lexicon_pos", "set_lexicon_pos", None, None)
            return
        t = np.ascontiguousarray(table, dtype=np.float32)
        c = np.ascontiguousarray(class_of_token, dtype=np.uint8)
        assert t.ndim == 2 and t.shape[1] == 5 and c.shape == (t.shape[0],)
        self._ck(self.lib.czc_set_lexicon_pos(self.h, t.ctypes.data, c.ctypes.data, t.shape[0]), "czc_set_lexicon_pos")
        self._record("lexicon_pos", "set_lexicon_pos", t, c)

    def set_lexicon(self, lex):
        m = np.ascontiguousarray(np.asarray(lex, dtype=np.float32).reshape(-1))
        self._ck(self.lib.czc_set_lexicon(self.h, m.ctypes.data, m.size), "czc_set_lexicon")
        self._record("lexicon", "set_lexicon", m)

    def set_pos(self, tag_of_token, template_masks):
        t = np.ascontiguousarray(np.asarray(tag_of_token, dtype=np.uint8).reshape(-1))
        m = np.ascontiguousarray(np.asarray(template_masks, dtype=np.uint16).reshape(-1))
        self._ck(self.lib.czc_set_pos(self.h, t.ctypes.data, t.size, m.ctypes.data, m.size), "czc_set_pos")
        self._record("pos", "set_pos", t, m)

    def set_control_callback(self, scorer):
        """czc_set_control_callback: `scorer(inp int32 [B,T], cand int32 [B,K], gen_idx) -> fp32 [B,K]` is called once per
        controlled step and replaces the control-score tables (conzic_amd/control.py: the reference's own nltk scorer on
        the decoded strings); None removes it.  An exception raised by the scorer fails the step and is re-raised by the
        generate / step call that triggered it."""
        if scorer is None:
            self._ck(self.lib.czc_set_control_callback(self.h, None, None), "czc_set_control_callback")
            self._ctl_fn = self._ctl_scorer = None
        else:
            def trampoline(_user, inp_p, cand_p, B, T, K, gen_idx, out_p):
                try:
                    inp = np.ctypeslib.as_array(inp_p, shape=(B, T)).copy()
                    cand = np.ctypeslib.as_array(cand_p, shape=(B, K)).copy()
                    sc = np.ascontiguousarray(scorer(inp, cand, int(gen_idx)), dtype=np.float32)
                    if sc.shape != (B, K):
                        raise ValueError(f"control scorer returned shape {sc.shape}, expected {(B, K)}")
                    np.ctypeslib.as_array(out_p, shape=(B, K))[...] = sc
                    return 0
                except BaseException as exc:  # noqa: BLE001 -- must not unwind through the C frames
                    self._ctl_error = exc
                    return 1
            fn = native.CONTROL_FN(trampoline)
            self._ck(self.lib.czc_set_control_callback(self.h, C.cast(fn, C.c_void_p), None), "czc_set_control_callback")
            self._ctl_fn, self._ctl_scorer = fn, scorer  # the C side keeps the pointer: keep the thunk alive
        self._ctl_error = None
        self._record("control_callback", "set_control_callback", scorer)

    def _raise_scorer_error(self):
        exc, self._ctl_error = getattr(self, "_ctl_error", None), None
        if exc is not None:
            raise exc

    def set_bridge(self, tables: BridgeArrays):
        st = tables.as_struct()
        self._ck(self.lib.czc_set_bridge(self.h, C.byref(st)), "czc_set_bridge")
        self._record("bridge", "set_bridge", tables)

    # ---- images / text ------------------------------------------------------------------------
    def encode_images(self, pixels) -> np.ndarray:
        if isinstance(pixels, np.ndarray):
            pixels = np.ascontiguousarray(pixels, dtype=np.float32)
        B = int(pixels.shape[0])
        out = np.empty((B, self.clip_cfg.proj), dtype=np.float32)
        self._ck(self.lib.czc_encode_images(self.h, _ptr(pixels), B, out.ctypes.data), "czc_encode_images")
        return out

    def preprocess_u8(self, rgb, slot: int = 0, want_pixels: bool = False, mean=None, std=None):
        """CLIPProcessor geometry on the device (czc_preprocess_u8): rgb uint8 [H,W,3] -> staged slot `slot`;
        returns the fp32 [3,S,S] pixels when want_pixels."""
        from .synth import CLIP_MEAN, CLIP_STD
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError("rgb must be uint8 [H, W, 3]")
        m = np.ascontiguousarray(CLIP_MEAN if mean is None else mean, dtype=np.float32)
        d = np.ascontiguousarray(CLIP_STD if std is None else std, dtype=np.float32)
        S = self.clip_cfg.v_image
        out = np.empty((3, S, S), dtype=np.float32) if want_pixels else None
        self._ck(self.lib.czc_preprocess_u8(self.h, rgb.ctypes.data, rgb.shape[0], rgb.shape[1], m.ctypes.data, d.ctypes.data,
                                            int(slot), out.ctypes.data if want_pixels else None), "czc_preprocess_u8")
        return out

    def encode_staged(self, B: int) -> np.ndarray:
        out = np.empty((int(B), self.clip_cfg.proj), dtype=np.float32)
        self._ck(self.lib.czc_encode_staged(self.h, int(B), out.ctypes.data), "czc_encode_staged")
        return out

    def encode_pil(self, images, mean=None, std=None) -> np.ndarray:
        """PIL images / uint8 arrays -> image_embeds, geometry and normalisation on the device."""
        if not isinstance(images, (list, tuple)):
            images = [images]
        for i, im in enumerate(images):
            if not isinstance(im, np.ndarray):
                im = np.asarray(im.convert("RGB"))
            self.preprocess_u8(im, i, mean=mean, std=std)
        return self.encode_staged(len(images))

    def preprocess_regions_u8(self, rgb, boxes, slot0: int = 0, want_pixels: bool = False, mean=None, std=None):
        """N boxes of one image in one call (czc_preprocess_regions_u8): rgb uint8 [H,W,3], boxes int [N,4] = x0, y0, x1, y1
        (PIL's crop convention) -> staged slots slot0 .. slot0 + N - 1, each what preprocess_u8 gives for rgb[y0:y1, x0:x1];
        returns the fp32 [N,3,S,S] pixels when want_pixels."""
        from .synth import CLIP_MEAN, CLIP_STD
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError("rgb must be uint8 [H, W, 3]")
        bx = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
        if bx.size and np.abs(bx).max() >= 2 ** 31:
            raise ValueError("a box coordinate outside int32")
        bx = np.ascontiguousarray(bx, dtype=np.int32)
        m = np.ascontiguousarray(CLIP_MEAN if mean is None else mean, dtype=np.float32)
        d = np.ascontiguousarray(CLIP_STD if std is None else std, dtype=np.float32)
        S = self.clip_cfg.v_image
        out = np.empty((bx.shape[0], 3, S, S), dtype=np.float32) if want_pixels else None
        self._ck(self.lib.czc_preprocess_regions_u8(self.h, rgb.ctypes.data, rgb.shape[0], rgb.shape[1], bx.ctypes.data,
                                                    bx.shape[0], m.ctypes.data, d.ctypes.data, int(slot0),
                                                    out.ctypes.data if want_pixels else None), "czc_preprocess_regions_u8")
        return out

    def encode_regions(self, image, boxes, mean=None, std=None) -> np.ndarray:
        """PIL image / uint8 array and N boxes -> image_embeds [N, proj]: the regions call at slot 0, then encode_staged(N);
        equal to encode_pil of the N host crops bit for bit (same pixels, same batch shape)."""
        if not isinstance(image, np.ndarray):
            image = np.asarray(image.convert("RGB"))
        n = int(np.size(boxes)) // 4
        self.preprocess_regions_u8(image, boxes, 0, mean=mean, std=std)
        return self.encode_staged(n)

    def set_image_embeds(self, embeds):
        e = np.ascontiguousarray(embeds, dtype=np.float32)
        self._ck(self.lib.czc_set_image_embeds(self.h, e.ctypes.data, e.shape[0]), "czc_set_image_embeds")

    def encode_text(self, clip_ids: np.ndarray, clip_len: np.ndarray) -> np.ndarray:
        n = int(clip_ids.shape[0])
        ids = np.full((n, native.CLIP_MAX_LEN), self.clip_cfg.eos_id, dtype=np.int32)
        ids[:, : clip_ids.shape[1]] = clip_ids
        ln = np.ascontiguousarray(clip_len, dtype=np.int32)
        out = np.empty((n, self.clip_cfg.proj), dtype=np.float32)
        self._ck(self.lib.czc_encode_text(self.h, ids.ctypes.data, ln.ctypes.data, n, out.ctypes.data), "czc_encode_text")
        return out

    # ---- hot path --------------------------------------------------------------------------------
    @staticmethod
    def hyper(alpha, beta, temperature, gamma=None, negative=False, control=None) -> native.Hyper:
        """control: None -> 'sentiment' when gamma is given (back-compat), else 'sentiment' | 'pos'."""
        h = native.Hyper()
        h.alpha, h.beta = float(alpha), float(beta)
        h.gamma = float(gamma) if gamma is not None else 0.0
        h.temperature = 1.0 if temperature is None else float(temperature)
        if gamma is None:
            h.control = 0
        else:
            h.control = 2 if control == "pos" else 1
        h.negative = 1 if negative else 0
        return h

    def step(self, inp: np.ndarray, gen_idx: int, top_k: int, hyper: native.Hyper, n_mask: int = 1,
             dot_allowed: bool = False, want: Sequence[str] = ("probs", "idxs", "cand_ids", "clip_ids", "clip_len",
                                                               "clip_score", "clip_ref", "final_score", "best",
                                                               "best_cos")) -> Dict[str, np.ndarray]:
        """One position-step on int32 `inp` [B,T] (updated in place).  Returns the requested tensors."""
        assert inp.dtype == np.int32 and inp.flags.c_contiguous
        B, T = inp.shape
        K = top_k
        V = self.cfg.bert_vocab
        shapes = dict(probs=((B, K), np.float32), idxs=((B, K), np.int32), cand_ids=((B, K), np.int32),
                      clip_ids=((B * K, native.CLIP_MAX_LEN), np.int32), clip_len=((B * K,), np.int32),
                      clip_score=((B, K), np.float32), clip_ref=((B, K), np.float32), senti_raw=((B, K), np.float32),
                      repeats=((B, K), np.float32), final_score=((B, K), np.float32), best=((B,), np.int32),
                      best_cos=((B,), np.float32), logits=((B, V), np.float32))
        out = native.StepOut()
        res = {}
        for name in want:
            shp, dt = shapes[name]
            res[name] = np.empty(shp, dtype=dt)
            setattr(out, name, res[name].ctypes.data)
        rc = self.lib.czc_step(self.h, inp.ctypes.data, B, T, gen_idx, n_mask, 1 if dot_allowed else 0, K,
                               C.byref(hyper), C.byref(out))
        if rc:
            self._raise_scorer_error()
        self._ck(rc, "czc_step")
        return res

    def generate(self, B: int, init_ids: Sequence[int], L: int, seed_len: int, top_k: int, positions: Sequence[int],
                 hyper: native.Hyper, n_mask: Optional[Sequence[int]] = None, snapshot_every: Optional[int] = None,
                 want_cos: bool = True):
        """Whole *_generation call.  Returns (ids int32 [S,B,T], cos fp32 [S,B]) per snapshot (cos None with want_cos=False:
        the C ABI's out_cos == NULL)."""
        init = np.ascontiguousarray(init_ids, dtype=np.int32)
        T = init.size
        pos = np.ascontiguousarray(positions, dtype=np.int32)
        nm = None if n_mask is None else np.ascontiguousarray(n_mask, dtype=np.int32)
        every = snapshot_every or L
        S = len(pos) // every
        ids = np.empty((S, B, T), dtype=np.int32)
        cos = np.empty((S, B), dtype=np.float32) if want_cos else None
        rc = self.lib.czc_generate(self.h, B, T, L, seed_len, init.ctypes.data, top_k, len(pos), pos.ctypes.data,
                                   None if nm is None else nm.ctypes.data, every, C.byref(hyper),
                                   ids.ctypes.data, None if cos is None else cos.ctypes.data)
        if rc:
            self._raise_scorer_error()
        self._ck(rc, "czc_generate")
        return ids, cos

    def _rows_call(self, name: str, call, init, positions, seed_len: int, L: Optional[int] = None, lens=None, need_lens: bool = False,
                   hypers=_ABSENT, draws=None, groups=None, rivals=None, deltas=_ABSENT, sets=None, set_of_row=None,
                   image_of_row=None, n_mask=None, snapshot_every: Optional[int] = None, want_cos: bool = True):
        """The one path of every generate_rows* method: checked, contiguous arrays of whatever per-row arguments the method has
        (`name` goes into the ValueError texts), the snapshot interval, the two outputs, then czc_<name>(handle, *call(a)), where
        `a` holds the sizes and the pointers (None = NULL), and the error check.  A new per-row argument is normalised here."""
        pos = np.ascontiguousarray(positions, dtype=np.int32)
        init = np.ascontiguousarray(init, dtype=np.int32)
        if pos.ndim != 2 or pos.shape[1] < 1:
            raise ValueError(f"{name}: positions must be [n_steps, R]")
        n_steps, R = pos.shape
        if name == "generate_rows":   # one start row [T] for every row
            T = init.size
        elif init.ndim != 2 or init.shape[0] != R or init.shape[1] < 1:
            raise ValueError(f"{name}: init_rows must be [R, T] with R = {R}, got {init.shape}")
        else:
            T = init.shape[1]
        if need_lens and lens is None:
            raise TypeError(f"{name}: lens is required")
        ln = _row_vector(name, "lens", lens, R)
        hp = None if hypers is _ABSENT else hyper_array(hypers)
        if hp is not None and len(hp) != R:
            raise ValueError(f"{name}: hypers has {len(hp)} entries for {R} rows")
        dr = None if draws is None else draw_array(draws)
        if dr is not None and len(dr) != R:
            raise ValueError(f"{name}: draws has {len(dr)} entries for {R} rows")
        gr = _row_vector(name, "groups", groups, R)
        ior = _row_vector(name, "image_of_row", image_of_row, R)
        rv = _rival_table(name, rivals, R)
        dl = None if deltas is _ABSENT else _row_vector(name, "deltas", np.zeros((R,), np.float32) if deltas is None else deltas, R,
                                                        dtype=np.float32)
        nm = _row_vector(name, "n_mask", n_mask, n_steps, "steps")
        so = _row_vector(name, "set_of_row", set_of_row, R)
        bits = None if sets is None else _vocab_sets(name, sets, int(self.cfg.bert_vocab))
        every = snapshot_every or (L if L is not None else max(int(ln.max()) if ln is not None else T - seed_len - 1, 1))
        S = n_steps // every
        ids = np.empty((S, R, T), dtype=np.int32)
        cos = np.empty((S, R), dtype=np.float32) if want_cos else None
        a = SimpleNamespace(R=R, T=T, n_steps=n_steps, every=every, init=_ptr(init), pos=_ptr(pos), lens=_ptr(ln), hypers=hp, draws=dr,
                            groups=_ptr(gr), ior=_ptr(ior), rivals=_ptr(rv), M=0 if rv is None else int(rv.shape[1]), deltas=_ptr(dl),
                            sets=_ptr(bits), n_sets=0 if bits is None else int(bits.shape[0]), set_of_row=_ptr(so),
                            n_mask=_ptr(nm), ids=_ptr(ids), cos=_ptr(cos))
        rc = getattr(self.lib, "czc_" + name)(self.h, *call(a))
        if rc:
            self._raise_scorer_error()
        self._ck(rc, "czc_" + name)
        return ids, cos

    def generate_rows(self, init_ids: Sequence[int], L: int, seed_len: int, top_k: int, positions, hyper: native.Hyper,
                      image_of_row: Optional[Sequence[int]] = None, n_mask: Optional[Sequence[int]] = None,
                      snapshot_every: Optional[int] = None, want_cos: bool = True):
        """czc_generate_rows: `positions` int [n_steps, R], row r visits positions[s][r] at step s and polishes a caption for
        resident image image_of_row[r] (None: row r = image r).  Returns (ids int32 [S,R,T], cos fp32 [S,R]) per snapshot."""
        return self._rows_call("generate_rows", lambda a: (a.R, a.T, L, seed_len, a.init, a.ior, top_k, a.n_steps, a.pos, a.n_mask, a.every,
                                                           C.byref(hyper), a.ids, a.cos),
                               init_ids, positions, seed_len, L=L, image_of_row=image_of_row, n_mask=n_mask,
                               snapshot_every=snapshot_every, want_cos=want_cos)

    def generate_rows_from(self, init_rows, L: int, seed_len: int, top_k: int, positions, hyper: native.Hyper,
                           image_of_row: Optional[Sequence[int]] = None, n_mask: Optional[Sequence[int]] = None,
                           snapshot_every: Optional[int] = None, want_cos: bool = True):
        """czc_generate_rows_from: generate_rows with a start row per row (`init_rows` int [R, T]: infilling, resume, polishing a
        draft) and positions that may be native.POS_IDLE (the row sits that step out).  Returns (ids int32 [S,R,T], cos fp32
        [S,R]) per snapshot; cos is 0 while a row has not run a step yet."""
        return self._rows_call("generate_rows_from", lambda a: (a.R, a.T, L, seed_len, a.init, a.ior, top_k, a.n_steps, a.pos, a.n_mask,
                                                                a.every, C.byref(hyper), a.ids, a.cos),
                               init_rows, positions, seed_len, L=L, image_of_row=image_of_row, n_mask=n_mask,
                               snapshot_every=snapshot_every, want_cos=want_cos)

    def generate_rows_len(self, init_rows, lens, seed_len: int, top_k: int, positions, hyper: native.Hyper,
                          image_of_row: Optional[Sequence[int]] = None, n_mask: Optional[Sequence[int]] = None,
                          snapshot_every: Optional[int] = None, want_cos: bool = True):
        """czc_generate_rows_len: generate_rows_from with a sentence length per row.  `init_rows` int [R, T] (T the stride: row r
        holds seed_len + lens[r] + 1 tokens, then id 0), `lens` int [R], `positions` int [n_steps, R] with positions[s][r] in
        [0, lens[r]) or native.POS_IDLE.  Returns (ids int32 [S,R,T], cos fp32 [S,R]) per snapshot (snapshot_every defaults to
        the longest length); the padding tails stay 0."""
        return self._rows_call("generate_rows_len", lambda a: (a.R, a.T, seed_len, a.init, a.lens, a.ior, top_k, a.n_steps, a.pos, a.n_mask,
                                                               a.every, C.byref(hyper), a.ids, a.cos),
                               init_rows, positions, seed_len, lens=lens, need_lens=True, image_of_row=image_of_row, n_mask=n_mask,
                               snapshot_every=snapshot_every, want_cos=want_cos)

    def generate_rows_hp(self, init_rows, lens, seed_len: int, top_k: int, positions, hypers: Sequence[native.Hyper],
                         image_of_row: Optional[Sequence[int]] = None, n_mask: Optional[Sequence[int]] = None,
                         snapshot_every: Optional[int] = None, want_cos: bool = True):
        """czc_generate_rows_hp: generate_rows_len with a native.Hyper per row (`hypers`, R entries: row r's own temperature,
        alpha, beta, gamma, control and negative).  `lens` None: every row has T - seed_len - 1 positions (the shape of
        generate_rows_from).  Returns (ids int32 [S,R,T], cos fp32 [S,R]) per snapshot."""
        return self._rows_call("generate_rows_hp", lambda a: (a.R, a.T, seed_len, a.init, a.lens, a.ior, top_k, a.n_steps, a.pos, a.n_mask,
                                                              a.every, a.hypers, a.ids, a.cos),
                               init_rows, positions, seed_len, lens=lens, hypers=hypers, image_of_row=image_of_row, n_mask=n_mask,
                               snapshot_every=snapshot_every, want_cos=want_cos)

    def generate_rows_draw(self, init_rows, lens, seed_len: int, top_k: int, positions, hypers: Sequence[native.Hyper],
                           draws: Optional[Sequence[native.Draw]], image_of_row: Optional[Sequence[int]] = None,
                           n_mask: Optional[Sequence[int]] = None, snapshot_every: Optional[int] = None, want_cos: bool = True):
        """czc_generate_rows_draw: generate_rows_hp with a native.Draw per row (`draws`, R entries or None: row r's seed, tau and
        step offset).  A row with tau > 0 draws its winner from softmax_K(final_score / tau) with a counter-based generator keyed
        by its seed; tau == 0 keeps the first argmax.  Returns (ids int32 [S,R,T], cos fp32 [S,R]) per snapshot."""
        return self._rows_call("generate_rows_draw", lambda a: (a.R, a.T, seed_len, a.init, a.lens, a.ior, top_k, a.n_steps, a.pos, a.n_mask,
                                                                a.every, a.hypers, a.draws, a.ids, a.cos),
                               init_rows, positions, seed_len, lens=lens, hypers=hypers, draws=draws, image_of_row=image_of_row,
                               n_mask=n_mask, snapshot_every=snapshot_every, want_cos=want_cos)

    def generate_rows_tied(self, init_rows, lens, seed_len: int, top_k: int, positions, hypers: Sequence[native.Hyper],
                           draws: Optional[Sequence[native.Draw]], groups: Optional[Sequence[int]],
                           image_of_row: Optional[Sequence[int]] = None, snapshot_every: Optional[int] = None,
                           want_cos: bool = True):
        """czc_generate_rows_tied: generate_rows_draw with rows tied into groups (`groups` int [R], values in [0, R), or None:
        generate_rows_draw itself).  The rows of a group hold one sentence: after every step each row's winner is written
        into its siblings, so W rows polish W positions of one caption per step.  Every step masks one position.  Returns
        (ids int32 [S,R,T], cos fp32 [S,R]) per snapshot; with groups, cos is the score_rows cosine of the merged caption."""
        return self._rows_call("generate_rows_tied", lambda a: (a.R, a.T, seed_len, a.init, a.lens, a.ior, a.groups, top_k, a.n_steps, a.pos,
                                                                None, a.every, a.hypers, a.draws, a.ids, a.cos),
                               init_rows, positions, seed_len, lens=lens, hypers=hypers, draws=draws, groups=groups,
                               image_of_row=image_of_row, snapshot_every=snapshot_every, want_cos=want_cos)

    def score_rows(self, rows, seed_len: int, lens: Optional[Sequence[int]] = None,
                   image_of_row: Optional[Sequence[int]] = None) -> np.ndarray:
        """czc_score_rows: the CLIP cosine fp32 [R] of BERT-id `rows` int [R, T] (decoded as the step decodes them; row r stops
        at seed_len + lens[r] + 1 tokens) with resident image image_of_row[r] (None: row r = image r), all on the device."""
        if hasattr(rows, "data_ptr"):   # a contiguous int32 torch tensor, on the device or the host: scored where it lies
            if str(rows.dtype) != "torch.int32" or not rows.is_contiguous():
                raise ValueError("score_rows: a tensor must be contiguous int32")
            r = rows
        else:
            r = np.ascontiguousarray(rows, dtype=np.int32)
        if r.ndim != 2 or r.shape[0] < 1 or r.shape[1] < 1:
            raise ValueError(f"score_rows: rows must be [R, T], got {tuple(r.shape)}")
        R, T = int(r.shape[0]), int(r.shape[1])
        ln = _row_vector("score_rows", "lens", lens, R)
        ior = _row_vector("score_rows", "image_of_row", image_of_row, R)
        out = np.empty((R,), dtype=np.float32)
        self._ck(self.lib.czc_score_rows(self.h, _ptr(r), R, T, seed_len, _ptr(ln), _ptr(ior), out.ctypes.data), "czc_score_rows")
        return out

    def fluency_rows(self, rows, seed_len: int, lens: Optional[Sequence[int]] = None, temperature: float = 1.0) -> dict:
        """czc_fluency_rows: BERT's pseudo-log-likelihood of BERT-id `rows` int [R, T] (numpy, or a contiguous int32 torch tensor
        on the host or the device; row r has lens[r] words behind seed_len prompt tokens, None: T - seed_len - 1).  Returns
        dict(logp fp32 [R, Lmax], rank int32 [R, Lmax], pll fp32 [R]): log softmax(logits / temperature) at every word's own id
        with that word masked, the id's rank among the vocabulary (0 = BERT's first choice), and the sum per row; the columns
        behind a row's words hold 0.0 and -1."""
        if hasattr(rows, "data_ptr"):
            if str(rows.dtype) != "torch.int32" or not rows.is_contiguous():
                raise ValueError("fluency_rows: a tensor must be contiguous int32")
            r = rows
        else:
            r = np.ascontiguousarray(rows, dtype=np.int32)
        if r.ndim != 2 or r.shape[0] < 1 or r.shape[1] < 1:
            raise ValueError(f"fluency_rows: rows must be [R, T], got {tuple(r.shape)}")
        R, T = int(r.shape[0]), int(r.shape[1])
        ln = _row_vector("fluency_rows", "lens", lens, R)
        lmax = max(T - int(seed_len) - 1, 0)   # (the C ABI refuses Lmax < 1: the buffers only have to exist)
        logp, rank = np.empty((R, lmax), dtype=np.float32), np.empty((R, lmax), dtype=np.int32)
        pll = np.empty((R,), dtype=np.float32)
        self._ck(self.lib.czc_fluency_rows(self.h, _ptr(r), R, T, int(seed_len), _ptr(ln), float(temperature), logp.ctypes.data,
                                           rank.ctypes.data, pll.ctypes.data), "czc_fluency_rows")
        return dict(logp=logp, rank=rank, pll=pll)

    def generate_rows_vs(self, init_rows, lens, seed_len: int, top_k: int, positions, hypers: Sequence[native.Hyper],
                         draws: Optional[Sequence[native.Draw]], groups: Optional[Sequence[int]], rivals, deltas,
                         image_of_row: Optional[Sequence[int]] = None, n_mask: Optional[Sequence[int]] = None,
                         snapshot_every: Optional[int] = None, want_cos: bool = True):
        """czc_generate_rows_vs: generate_rows_tied with rival images per row.  `rivals` int [R, M] (indices into the resident
        image batch, -1 = empty slot, filled slots first; None: generate_rows_tied itself) and `deltas` float [R]: row r adds
        deltas[r] * P(own image | candidate, among own image and rivals) to every candidate's fused score.  `n_mask` (span
        order) only without groups.  Returns (ids int32 [S,R,T], cos fp32 [S,R]) per snapshot."""
        return self._rows_call("generate_rows_vs", lambda a: (a.R, a.T, seed_len, a.init, a.lens, a.ior, a.groups, top_k, a.n_steps, a.pos,
                                                              a.n_mask, a.every, a.hypers, a.draws, a.rivals, a.M, a.deltas, a.ids, a.cos),
                               init_rows, positions, seed_len, lens=lens, hypers=hypers, draws=draws, groups=groups, rivals=rivals,
                               deltas=deltas, image_of_row=image_of_row, n_mask=n_mask, snapshot_every=snapshot_every, want_cos=want_cos)

    def generate_rows_vocab(self, init_rows, lens, seed_len: int, top_k: int, positions, hypers: Sequence[native.Hyper],
                            draws: Optional[Sequence[native.Draw]] = None, groups: Optional[Sequence[int]] = None, rivals=None,
                            deltas=None, sets=None, set_of_row: Optional[Sequence[int]] = None,
                            image_of_row: Optional[Sequence[int]] = None, n_mask: Optional[Sequence[int]] = None,
                            snapshot_every: Optional[int] = None, want_cos: bool = True):
        """czc_generate_rows_vocab: generate_rows_vs with a vocabulary set per row.  `sets` uint32 [n_sets, ceil(V / 32)] bitsets
        (bit i & 31 of word i >> 5 set = id i allowed; conzic_amd.vocab.pack / ban / allow build them) and `set_of_row` int [R],
        -1 = no set (None: generate_rows_vs itself).  In row r's masked softmax the mask factor of id i is token_mask[i] * bit(i),
        the '.' rule still on top.  Returns (ids int32 [S,R,T], cos fp32 [S,R]) per snapshot."""
        return self._rows_call("generate_rows_vocab", lambda a: (a.R, a.T, seed_len, a.init, a.lens, a.ior, a.groups, top_k, a.n_steps, a.pos,
                                                                 a.n_mask, a.every, a.hypers, a.draws, a.rivals, a.M, a.deltas, a.sets, a.n_sets,
                                                                 a.set_of_row, a.ids, a.cos),
                               init_rows, positions, seed_len, lens=lens, hypers=hypers, draws=draws, groups=groups, rivals=rivals,
                               deltas=deltas, sets=sets, set_of_row=set_of_row, image_of_row=image_of_row, n_mask=n_mask,
                               snapshot_every=snapshot_every, want_cos=want_cos)

    def score_rows_vs(self, rows, seed_len: int, rivals, lens: Optional[Sequence[int]] = None,
                      image_of_row: Optional[Sequence[int]] = None):
        """czc_score_rows_vs: (cos fp32 [R], disc fp32 [R]) of BERT-id `rows` int [R, T]: score_rows' cosine, bit for bit, and
        P(own image | row) among the row's own image and its `rivals` (int [R, M], -1 = empty; None: disc is 1 everywhere)."""
        r = np.ascontiguousarray(rows, dtype=np.int32)
        if r.ndim != 2 or r.shape[0] < 1 or r.shape[1] < 1:
            raise ValueError(f"score_rows_vs: rows must be [R, T], got {tuple(r.shape)}")
        R, T = int(r.shape[0]), int(r.shape[1])
        ln = _row_vector("score_rows_vs", "lens", lens, R)
        ior = _row_vector("score_rows_vs", "image_of_row", image_of_row, R)
        rv = _rival_table("score_rows_vs", rivals, R)
        cos, disc = np.empty((R,), dtype=np.float32), np.empty((R,), dtype=np.float32)
        self._ck(self.lib.czc_score_rows_vs(self.h, r.ctypes.data, R, T, seed_len, _ptr(ln), _ptr(ior), _ptr(rv),
                                            0 if rv is None else int(rv.shape[1]), cos.ctypes.data, disc.ctypes.data),
                 "czc_score_rows_vs")
        return cos, disc

    def similarity(self, image_embeds, text_embeds, K: int):
        """clip/clip.py:86-98: (softmax_K(cos * exp(logit_scale)), cos), both [B, K], from un-normalised embeddings."""
        ie = np.ascontiguousarray(image_embeds, np.float32)
        te = np.ascontiguousarray(text_embeds, np.float32)
        if ie.ndim != 2 or te.ndim != 2 or ie.shape[1] != self.clip_cfg.proj or te.shape[1] != self.clip_cfg.proj:
            raise ValueError(f"similarity: embeddings must be [*, {self.clip_cfg.proj}], got {ie.shape} and {te.shape}")
        B = ie.shape[0]
        assert te.shape == (B * K, ie.shape[1]), (te.shape, ie.shape, K)
        cs, cr = np.empty((B, K), np.float32), np.empty((B, K), np.float32)
        self._ck(self.lib.czc_similarity(self.h, ie.ctypes.data, te.ctypes.data, B, K, cs.ctypes.data, cr.ctypes.data), "czc_similarity")
        return cs, cr

    # ---- caption retrieval ---------------------------------------------------------------------
    def index_set(self, embeds):
        """czc_index_set: fp32 [n, proj] un-normalised text embeddings (numpy, or a device tensor) become this engine's index
        (a replica has none of its own)."""
        if isinstance(embeds, np.ndarray) or not hasattr(embeds, "data_ptr"):
            embeds = np.ascontiguousarray(embeds, dtype=np.float32)
        if embeds.ndim != 2 or int(embeds.shape[1]) != self.clip_cfg.proj:
            raise ValueError(f"index rows must be [n, {self.clip_cfg.proj}], got {tuple(embeds.shape)}")
        self._ck(self.lib.czc_index_set(self.h, _ptr(embeds), int(embeds.shape[0])), "czc_index_set")

    def index_clear(self):
        self._ck(self.lib.czc_index_set(self.h, None, 0), "czc_index_set")

    def index_size(self) -> int:
        n = C.c_int64()
        self._ck(self.lib.czc_index_size(self.h, C.byref(n)), "czc_index_size")
        return int(n.value)

    def index_search(self, image_embeds=None, k: int = 1, Q: Optional[int] = None):
        """czc_index_search: (ids int32 [Q, k], cosines fp32 [Q, k]) ordered by (cosine descending, id ascending).
        image_embeds fp32 [Q, proj] un-normalised (numpy or device tensor); None = the first Q resident image embeddings."""
        if image_embeds is None:
            if Q is None:
                raise ValueError("index_search(None) needs Q, the number of resident image embeddings to search with")
        else:
            if isinstance(image_embeds, np.ndarray) or not hasattr(image_embeds, "data_ptr"):
                image_embeds = np.ascontiguousarray(image_embeds, dtype=np.float32)
            if image_embeds.ndim != 2 or int(image_embeds.shape[1]) != self.clip_cfg.proj:
                raise ValueError(f"queries must be [Q, {self.clip_cfg.proj}], got {tuple(image_embeds.shape)}")
            Q = int(image_embeds.shape[0])
        # (the C ABI checks Q and k: wrong values come back as CZC_ERR_ARG; the buffers only have to exist)
        ids = np.empty((max(int(Q), 0), max(int(k), 0)), dtype=np.int32)
        cos = np.empty(ids.shape, dtype=np.float32)
        self._ck(self.lib.czc_index_search(self.h, _ptr(image_embeds), int(Q), int(k), ids.ctypes.data, cos.ctypes.data),
                 "czc_index_search")
        return ids, cos

    def set_option(self, name: str, value: int):
        self._ck(self.lib.czc_set_option(self.h, name.encode(), int(value)), f"czc_set_option({name})")
        self._record("option:" + name, "set_option", name, int(value))

    def get_option(self, name: str) -> int:
        """An option as the engine holds it (czc_get_option; also the derived read-only values, e.g. the guard's trip point in
        force inside czc_generate: "refine_guard_generate_x1e6")."""
        v = C.c_int()
        self._ck(self.lib.czc_get_option(self.h, name.encode(), C.byref(v)), f"czc_get_option({name})")
        return int(v.value)

    # ---- measurement ------------------------------------------------------------------------------
    def profile(self, on):
        """False/0 off, True/1 every kernel class, 2 only the CLIP-text linear layers (cheap: the roofline family)."""
        self._ck(self.lib.czc_profile_enable(self.h, int(on)), "czc_profile_enable")

    def profile_reset(self):
        self._ck(self.lib.czc_profile_reset(self.h), "czc_profile_reset")

    def profile_get(self, kind: str):
        ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
        self._ck(self.lib.czc_profile_get(self.h, kind.encode(), C.byref(ms), C.byref(n), C.byref(fl)), "czc_profile_get")
        return dict(ms=ms.value, launches=n.value, flops=fl.value)

    def stats(self):
        a, b, c_, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        self._ck(self.lib.czc_stats(self.h, C.byref(a), C.byref(b), C.byref(c_), C.byref(d)), "czc_stats")
        rs, rr = C.c_int64(), C.c_int64()
        self._ck(self.lib.czc_refine_stats(self.h, C.byref(rs), C.byref(rr)), "czc_refine_stats")
        g, gi = C.c_int64(), C.c_int64()
        self._ck(self.lib.czc_refine_gate_stats(self.h, C.byref(g), C.byref(gi)), "czc_refine_gate_stats")
        dd = C.c_int64()
        self._ck(self.lib.czc_dedup_stats(self.h, C.byref(dd), None), "czc_dedup_stats")
        return dict(clip_rows=a.value, clip_seqs=b.value, bert_rows=c_.value, steps=d.value, refine_seqs=rs.value,
                    refine_rows=rr.value, gated_image_steps=g.value, gate_image_steps=gi.value, dedup_seqs=dd.value)

    def memo_stats(self):
        """Option "memo" (czc_memo_stats): image-steps of memo-on czc_generate calls since profile_reset, and how many of them
        took a memo entry instead of running."""
        h, n = C.c_int64(), C.c_int64()
        self._ck(self.lib.czc_memo_stats(self.h, C.byref(h), C.byref(n)), "czc_memo_stats")
        return dict(hit_image_steps=h.value, image_steps=n.value)

    def memo_rows_stats(self):
        """Option "memo_rows" (czc_memo_rows_stats): row-steps of czc_generate_rows calls made with the option on since
        profile_reset, and how many of them took their entry instead of running."""
        h, n = C.c_int64(), C.c_int64()
        self._ck(self.lib.czc_memo_rows_stats(self.h, C.byref(h), C.byref(n)), "czc_memo_rows_stats")
        return dict(hit_row_steps=h.value, row_steps=n.value)

    def refine_guard(self, reset: bool = True):
        """(max |screening error - mean| seen on re-encoded candidates, image-steps above the trip point) of a
        CZC_PREC_REFINE engine since the last reset (czc_refine_guard)."""
        dev, trips = C.c_float(), C.c_int64()
        self._ck(self.lib.czc_refine_guard(self.h, 1 if reset else 0, C.byref(dev), C.byref(trips)), "czc_refine_guard")
        return dict(max_dev=float(dev.value), tripped=int(trips.value))

    def sync(self):
        self._ck(self.lib.czc_sync(self.h), "czc_sync")

    def profile_intervals(self, kind: str, ref: Optional["Engine"] = None) -> np.ndarray:
        """[n, 2] start / end (ms) of every launch of class `kind` since profile_reset, on the clock that starts at
        `ref`'s profile_reset (default: this engine's)."""
        ref = ref or self
        n = C.c_int(0)
        self._ck(self.lib.czc_profile_intervals(self.h, ref.h, kind.encode(), None, None, 0, C.byref(n)), "czc_profile_intervals")
        a = np.empty(max(n.value, 1), np.float64)
        b = np.empty(max(n.value, 1), np.float64)
        self._ck(self.lib.czc_profile_intervals(self.h, ref.h, kind.encode(), a.ctypes.data, b.ctypes.data, n.value,
                                                C.byref(n)), "czc_profile_intervals")
        return np.stack([a[: n.value], b[: n.value]], axis=1)


def union_ms(intervals: Sequence[np.ndarray]) -> float:
    """Total length of the union of [start, end] intervals (ms) from one or more engines on a common clock."""
    iv = np.concatenate([x for x in intervals if len(x)], axis=0) if any(len(x) for x in intervals) else np.zeros((0, 2))
    if not len(iv):
        return 0.0
    iv = iv[np.argsort(iv[:, 0])]
    total, cur_s, cur_e = 0.0, iv[0, 0], iv[0, 1]
    for s_, e_ in iv[1:]:
        if s_ > cur_e:
            total += cur_e - cur_s
            cur_s, cur_e = s_, e_
        else:
            cur_e = max(cur_e, e_)
    return float(total + (cur_e - cur_s))


class EngineGroup:
    """One engine plus replicas over the same weights, each on its own HIP stream, polishing disjoint contiguous image
    sub-batches concurrently from host threads (the C calls release the GIL).  Images are independent
    (gen_utils.py:64-81), so the captions are the single-engine ones image for image; what changes is that one
    sub-batch's small launches (BERT, top-K, LayerNorm, attention) and the tail rounds of its persistent GEMMs overlap
    the other's big launches: +5 % captions/s at 256 images with two streams.  Below `min_images` per
    stream the batch is not split."""

    def __init__(self, engine: Engine, streams: int = 2, min_images: int = 32):
        from concurrent.futures import ThreadPoolExecutor
        self.engines = [engine] + [engine.replica() for _ in range(max(1, int(streams)) - 1)]
        self.min_images = int(min_images)
        self._pool = ThreadPoolExecutor(max_workers=len(self.engines)) if len(self.engines) > 1 else None
        self._full_embeds = None
        self._encoded = None  # what encode_images returned (un-normalised, as set_image_embeds takes them): generate_rows re-deals it by row

    @property
    def streams(self) -> int:
        return len(self.engines)

    def parts(self, B: int):
        """Contiguous (lo, hi) image ranges, one per engine used."""
        n = max(1, min(len(self.engines), B // max(self.min_images, 1)))
        base, rem = divmod(B, n)
        out, lo = [], 0
        for r in range(n):
            hi = lo + base + (1 if r < rem else 0)
            out.append((lo, hi))
            lo = hi
        return out

    def _run(self, jobs):
        if len(jobs) == 1 or self._pool is None:
            return [j() for j in jobs]
        futs = [self._pool.submit(j) for j in jobs]
        return [f.result() for f in futs]

    def encode_images(self, pixels) -> np.ndarray:
        B = int(pixels.shape[0])
        parts = self.parts(B)
        outs = self._run([(lambda e=e, lo=lo, hi=hi: e.encode_images(pixels[lo:hi])) for e, (lo, hi) in zip(self.engines, parts)])
        self._full_embeds = None  # every engine now holds its own slice
        self._resident = parts
        self._encoded = np.concatenate(outs, axis=0)  # generate_rows hands every member the embeds of its own rows
        return self._encoded

    def set_image_embeds(self, embeds):
        self._full_embeds = np.ascontiguousarray(embeds, dtype=np.float32)
        self._resident = None
        self._encoded = None

    def generate(self, B: int, init_ids, L: int, seed_len: int, top_k: int, positions, hyper, n_mask=None,
                 snapshot_every=None):
        parts = self.parts(B)
        if self._full_embeds is not None:
            for e, (lo, hi) in zip(self.engines, parts):
                e.set_image_embeds(self._full_embeds[lo:hi])
        elif getattr(self, "_resident", None) != parts:
            raise NativeError("EngineGroup.generate: encode_images / set_image_embeds of the same batch first")
        outs = self._run([(lambda e=e, lo=lo, hi=hi: e.generate(hi - lo, init_ids, L, seed_len, top_k, positions, hyper,
                                                                n_mask=n_mask, snapshot_every=snapshot_every))
                          for e, (lo, hi) in zip(self.engines, parts)])
        return np.concatenate([o[0] for o in outs], axis=1), np.concatenate([o[1] for o in outs], axis=1)

    def _split_rows(self, name: str, run, init, positions, seed_len: int, L: Optional[int] = None, lens=None, hypers=None, draws=None,
                    groups=None, rivals=None, deltas=None, set_of_row=None, image_of_row=None, snapshot_every=None,
                    want_cos: bool = True, images: str = "rows"):
        """The one path of every generate_rows* method of the group: check the per-row arguments the method has, work out the
        snapshot interval of the whole call, deal the rows over the members (contiguously, or on group boundaries with `groups`),
        hand every member its images, call run(member, p) -- p holds the member's slice of every per-row argument (rows, init,
        lens, pos, hypers, draws, groups renumbered into [0, its row count), rivals, deltas, set_of_row, ior) and `every` -- and put the
        results back by row index.  images: "rows" = the embeds of its own rows, p.ior None (the identity); "unique" = the embeds
        of the images its rows name and p.ior into them; "whole" = the whole batch and the caller's indices (rivals may name any
        image).  The normalisation is per row, so a row's embedding has the bits the whole batch had.  A new per-row argument is
        checked and sliced here."""
        pos = np.ascontiguousarray(positions, dtype=np.int32)
        if pos.ndim != 2:
            raise ValueError(f"{name}: positions must be [n_steps, R]")
        R = pos.shape[1]
        if name != "generate_rows":   # (its one start row goes to every member as it is)
            init = np.ascontiguousarray(init, dtype=np.int32)
            if init.ndim != 2 or init.shape[0] != R:
                raise ValueError(f"{name}: init_rows must be [R, T] with R = {R}, got {init.shape}")
        ln = None if lens is None else np.ascontiguousarray(lens, dtype=np.int32).reshape(-1)
        hps, drs = None if hypers is None else list(hypers), None if draws is None else list(draws)
        for what, v in (("lens", ln), ("hypers", hps), ("draws", drs)):
            if v is not None and len(v) != R:
                raise ValueError(f"{name}: {what} has {len(v)} entries for {R} rows")
        gr = None if groups is None else np.asarray(groups, dtype=np.int64).reshape(-1)
        if gr is not None:
            outside = gr.size == R and R and (gr.min() < 0 or gr.max() >= R)
            if name == "generate_rows_vs" and (gr.size != R or outside):
                raise NativeError("EngineGroup.generate_rows_vs: groups must hold R ids in [0, R)", code=native.ERR_ARG)
            if gr.size != R:
                raise ValueError(f"{name}: groups has {gr.size} entries for {R} rows")
            if outside:
                raise NativeError(f"EngineGroup.{name}: a group id outside [0, R)", code=native.ERR_ARG)
        rv = _rival_table(name, rivals, R)
        dl = None if rv is None else _row_vector(name, "deltas", np.zeros((R,), np.float32) if deltas is None else deltas, R, dtype=np.float32)
        so = _row_vector(name, "set_of_row", set_of_row, R)
        embeds = self._full_embeds if self._full_embeds is not None else self._encoded
        if embeds is None:
            raise NativeError(f"EngineGroup.{name}: encode_images / set_image_embeds first")
        ior = np.arange(R) if image_of_row is None else np.asarray(image_of_row, dtype=np.int64).reshape(-1)
        if ior.size != R or (R and (ior.min() < 0 or ior.max() >= embeds.shape[0])):
            raise NativeError(f"EngineGroup.{name}: image_of_row outside the resident image batch", code=native.ERR_ARG)
        every = snapshot_every or (L if L is not None else max(int(ln.max()) if ln is not None else init.shape[1] - seed_len - 1, 1))
        parts = self.tied_parts(gr) if gr is not None else [np.arange(lo, hi) for lo, hi in self.parts(R)]
        jobs = []
        for e, rows in zip(self.engines, parts):
            p = SimpleNamespace(rows=rows, every=every, init=init if name == "generate_rows" else init[rows],
                                lens=None if ln is None else ln[rows], pos=np.ascontiguousarray(pos[:, rows]),
                                hypers=None if hps is None else [hps[r] for r in rows], draws=None if drs is None else [drs[r] for r in rows],
                                groups=None if gr is None else np.unique(gr[rows], return_inverse=True)[1].astype(np.int32),
                                rivals=None if rv is None else rv[rows], deltas=None if dl is None else dl[rows],
                                set_of_row=None if so is None else so[rows], ior=None)
            if images == "rows":
                e.set_image_embeds(embeds[ior[rows]])
            elif images == "unique":
                imgs, img_c = np.unique(ior[rows], return_inverse=True)
                e.set_image_embeds(embeds[imgs])
                p.ior = img_c.astype(np.int32)
            else:
                e.set_image_embeds(embeds)
                p.ior = ior[rows].astype(np.int32)
            jobs.append(lambda e=e, p=p: run(e, p))
        # the members now hold other embeds than their image slices: a later generate() hands the slices over again
        self._full_embeds, self._resident = embeds, None
        outs = self._run(jobs)
        ids = np.empty((outs[0][0].shape[0], R, outs[0][0].shape[2]), dtype=np.int32)
        cos = np.empty(ids.shape[:2], dtype=np.float32) if want_cos else None
        for rows, (i, c) in zip(parts, outs):
            ids[:, rows] = i
            if want_cos:
                cos[:, rows] = c
        return ids, cos

    def generate_rows(self, init_ids, L: int, seed_len: int, top_k: int, positions, hyper, image_of_row=None, n_mask=None,
                      snapshot_every=None):
        """Engine.generate_rows with the rows split contiguously over the streams.  `image_of_row` is resolved here: every
        member gets the embeds of its own rows (the normalisation is per row, so they are the bits the whole batch had) and
        runs its rows with the identity."""
        return self._split_rows("generate_rows", lambda e, p: e.generate_rows(init_ids, L, seed_len, top_k, p.pos, hyper, n_mask=n_mask,
                                                                              snapshot_every=snapshot_every),
                                init_ids, positions, seed_len, L=L, image_of_row=image_of_row, snapshot_every=snapshot_every)

    def generate_rows_from(self, init_rows, L: int, seed_len: int, top_k: int, positions, hyper, image_of_row=None, n_mask=None,
                           snapshot_every=None):
        """Engine.generate_rows_from with the rows (start rows, positions, images) split contiguously over the streams, as
        generate_rows splits them."""
        return self._split_rows("generate_rows_from", lambda e, p: e.generate_rows_from(p.init, L, seed_len, top_k, p.pos, hyper, n_mask=n_mask,
                                                                                        snapshot_every=snapshot_every),
                                init_rows, positions, seed_len, L=L, image_of_row=image_of_row, snapshot_every=snapshot_every)

    def generate_rows_len(self, init_rows, lens, seed_len: int, top_k: int, positions, hyper, image_of_row=None, n_mask=None,
                          snapshot_every=None, want_cos: bool = True):
        """Engine.generate_rows_len with the rows (start rows, lengths, positions, images) split contiguously over the streams,
        as generate_rows_from splits them.  Every member keeps the whole call's stride and snapshot interval."""
        lens = np.ascontiguousarray(lens, dtype=np.int32)   # (required here: None is refused as the engine refuses it)
        return self._split_rows("generate_rows_len", lambda e, p: e.generate_rows_len(p.init, p.lens, seed_len, top_k, p.pos, hyper, n_mask=n_mask,
                                                                                      snapshot_every=p.every, want_cos=want_cos),
                                init_rows, positions, seed_len, lens=lens, image_of_row=image_of_row, snapshot_every=snapshot_every,
                                want_cos=want_cos)

    def generate_rows_hp(self, init_rows, lens, seed_len: int, top_k: int, positions, hypers, image_of_row=None, n_mask=None,
                         snapshot_every=None, want_cos: bool = True):
        """Engine.generate_rows_hp with the rows (start rows, lengths, positions, images, hyper-parameters) split contiguously over
        the streams, as generate_rows_len splits them.  Every member keeps the whole call's stride and snapshot interval."""
        return self._split_rows("generate_rows_hp", lambda e, p: e.generate_rows_hp(p.init, p.lens, seed_len, top_k, p.pos, p.hypers, n_mask=n_mask,
                                                                                    snapshot_every=p.every, want_cos=want_cos),
                                init_rows, positions, seed_len, lens=lens, hypers=list(hypers), image_of_row=image_of_row,
                                snapshot_every=snapshot_every, want_cos=want_cos)

    def generate_rows_draw(self, init_rows, lens, seed_len: int, top_k: int, positions, hypers, draws, image_of_row=None,
                           n_mask=None, snapshot_every=None, want_cos: bool = True):
        """Engine.generate_rows_draw with the rows split contiguously over the streams, as generate_rows_hp splits them.  A row's
        draw record travels with it and holds everything its draws depend on (seed, tau, step offset), so the result does not
        depend on the split."""
        return self._split_rows("generate_rows_draw", lambda e, p: e.generate_rows_draw(p.init, p.lens, seed_len, top_k, p.pos, p.hypers, p.draws,
                                                                                        n_mask=n_mask, snapshot_every=p.every, want_cos=want_cos),
                                init_rows, positions, seed_len, lens=lens, hypers=list(hypers), draws=draws, image_of_row=image_of_row,
                                snapshot_every=snapshot_every, want_cos=want_cos)

    def tied_parts(self, groups):
        """Row index arrays, one per engine used: the rows dealt over the streams on group boundaries only.  Groups go, in
        the order of their first rows, to the current part until it holds its share of the rows; a group is never cut."""
        gr = np.asarray(groups, dtype=np.int64).reshape(-1)
        R = gr.size
        n = max(1, min(len(self.engines), R // max(self.min_images, 1)))
        order, members = [], {}
        for r, g in enumerate(gr.tolist()):
            if g not in members:
                members[g] = []
                order.append(g)
            members[g].append(r)
        parts, cur, done = [], [], 0
        for g in order:
            cur += members[g]
            if len(parts) < n - 1 and done + len(cur) >= (len(parts) + 1) * R / n:
                parts.append(cur)
                done += len(cur)
                cur = []
        if cur:
            parts.append(cur)
        return [np.array(sorted(p), dtype=np.int64) for p in parts]

    def generate_rows_tied(self, init_rows, lens, seed_len: int, top_k: int, positions, hypers, draws, groups, image_of_row=None,
                           snapshot_every=None, want_cos: bool = True):
        """Engine.generate_rows_tied with the rows split over the streams ON GROUP BOUNDARIES ONLY (tied_parts; groups None:
        generate_rows_draw's contiguous split).  A member gets the embeds of the images its rows name and its rows' image indices
        into them, so the rows of a group still share one image."""
        if groups is None:
            return self.generate_rows_draw(init_rows, lens, seed_len, top_k, positions, hypers, draws, image_of_row=image_of_row,
                                           snapshot_every=snapshot_every, want_cos=want_cos)
        return self._split_rows("generate_rows_tied", lambda e, p: e.generate_rows_tied(p.init, p.lens, seed_len, top_k, p.pos, p.hypers, p.draws,
                                                                                        p.groups, image_of_row=p.ior, snapshot_every=p.every,
                                                                                        want_cos=want_cos),
                                init_rows, positions, seed_len, lens=lens, hypers=list(hypers), draws=draws, groups=groups,
                                image_of_row=image_of_row, snapshot_every=snapshot_every, want_cos=want_cos, images="unique")

    def generate_rows_vs(self, init_rows, lens, seed_len: int, top_k: int, positions, hypers, draws, groups, rivals, deltas,
                         image_of_row=None, n_mask=None, snapshot_every=None, want_cos: bool = True):
        """Engine.generate_rows_vs with the rows split over the streams (on group boundaries where `groups` is given).  A rival
        may be any image of the batch, so every member holds the WHOLE resident batch and gets `image_of_row` and the rival
        indices unchanged -- unlike generate_rows, which deals out per-row embeddings.  The normalisation is per row, so a
        row's own embedding has the bits it has there."""
        if rivals is None and groups is None:
            return self.generate_rows_draw(init_rows, lens, seed_len, top_k, positions, hypers, draws, image_of_row=image_of_row,
                                           n_mask=n_mask, snapshot_every=snapshot_every, want_cos=want_cos)
        if rivals is None:
            return self.generate_rows_tied(init_rows, lens, seed_len, top_k, positions, hypers, draws, groups, image_of_row=image_of_row,
                                           snapshot_every=snapshot_every, want_cos=want_cos)
        return self._split_rows("generate_rows_vs", lambda e, p: e.generate_rows_vs(p.init, p.lens, seed_len, top_k, p.pos, p.hypers, p.draws,
                                                                                    p.groups, p.rivals, p.deltas, image_of_row=p.ior,
                                                                                    n_mask=n_mask, snapshot_every=p.every, want_cos=want_cos),
                                init_rows, positions, seed_len, lens=lens, hypers=list(hypers), draws=draws, groups=groups, rivals=rivals,
                                deltas=deltas, image_of_row=image_of_row, snapshot_every=snapshot_every, want_cos=want_cos, images="whole")

    def generate_rows_vocab(self, init_rows, lens, seed_len: int, top_k: int, positions, hypers, draws=None, groups=None, rivals=None,
                            deltas=None, sets=None, set_of_row=None, image_of_row=None, n_mask=None, snapshot_every=None,
                            want_cos: bool = True):
        """Engine.generate_rows_vocab with the rows split over the streams as generate_rows_vs splits them (every member holds the
        whole resident batch).  Every member gets the WHOLE table of bitsets and its own rows' indices into it, so an index means
        the same set on every stream."""
        return self._split_rows("generate_rows_vocab", lambda e, p: e.generate_rows_vocab(p.init, p.lens, seed_len, top_k, p.pos, p.hypers, p.draws,
                                                                                          p.groups, p.rivals, p.deltas, sets=sets,
                                                                                          set_of_row=p.set_of_row, image_of_row=p.ior,
                                                                                          n_mask=n_mask, snapshot_every=p.every, want_cos=want_cos),
                                init_rows, positions, seed_len, lens=lens, hypers=list(hypers), draws=draws, groups=groups, rivals=rivals,
                                deltas=deltas, set_of_row=set_of_row, image_of_row=image_of_row, snapshot_every=snapshot_every,
                                want_cos=want_cos, images="whole")

    def fluency_rows(self, rows, seed_len: int, lens=None, temperature: float = 1.0) -> dict:
        """Engine.fluency_rows on the parent engine, WITHOUT a split over the streams: the call needs no image embeds, a
        caption's result does not depend on its companions beyond the engine precision, and it is a scoring pass after the
        chains have ended, not part of them."""
        return self.engines[0].fluency_rows(rows, seed_len, lens=lens, temperature=temperature)

    # ---- the engine calls that apply to every member ----
    def set_option(self, name, value):
        self.engines[0].set_option(name, value)  # forwarded to the replicas

    def profile(self, on):
        for e in self.engines:
            e.profile(on)

    def profile_reset(self):
        for e in self.engines:
            e.profile_reset()

    def profile_get(self, kind: str):
        """Sum over the engines; `busy_ms` is the union of their launch intervals (what the GPU spent on the class)."""
        gs = [e.profile_get(kind) for e in self.engines]
        ref = self.engines[0]
        busy = union_ms([e.profile_intervals(kind, ref) for e in self.engines])
        return dict(ms=sum(g["ms"] for g in gs), launches=sum(g["launches"] for g in gs), flops=sum(g["flops"] for g in gs),
                    busy_ms=busy)

    def stats(self):
        ss = [e.stats() for e in self.engines]
        return {k: sum(s_[k] for s_ in ss) for k in ss[0]}

    def memo_stats(self):
        ms = [e.memo_stats() for e in self.engines]
        return {k: sum(m[k] for m in ms) for k in ms[0]}

    def memo_rows_stats(self):
        ms = [e.memo_rows_stats() for e in self.engines]
        return {k: sum(m[k] for m in ms) for k in ms[0]}

    def refine_guard(self, reset: bool = True):
        gs = [e.refine_guard(reset) for e in self.engines]
        return dict(max_dev=max(g["max_dev"] for g in gs), tripped=sum(g["tripped"] for g in gs))

    def close(self, parent: bool = True):
        """Close the replicas (and the thread pool); the first engine too unless parent=False."""
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
        head = self.engines[0]
        for r in self.engines[1:]:
            r.close()
            if r in head._replicas:
                head._replicas.remove(r)
        self.engines = [head]
        if parent:
            head.close()
