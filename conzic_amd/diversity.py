"""Caption diversity of one image's samples: Div-n, the number of distinct n-grams over the number of n-grams (Div-1 / Div-2 of
the diversity tables in the captioning literature), computed per image over its captions."""
from typing import Dict, List, Sequence


def tokenize(text: str) -> List[str]:
    """Lower-cased words: nltk.word_tokenize where nltk (and its tokenizer data) is there, else whitespace split."""
    text = text.lower()
    try:
        import nltk
        return list(nltk.word_tokenize(text))
    except Exception:   # no nltk, or nltk without its punkt data
        return text.split()


def distinct_n(captions: Sequence[str], ns: Sequence[int] = (1, 2)) -> Dict[int, float]:
    """{n: distinct n-grams / n-grams} over all `captions` of one image; 0.0 where the captions hold no n-gram."""
    toks = [tokenize(c) for c in captions]
    out = {}
    for n in ns:
        grams = [tuple(t[i:i + n]) for t in toks for i in range(len(t) - n + 1)]
        out[int(n)] = len(set(grams)) / len(grams) if grams else 0.0
    return out


def log_distinct(logger, img_name: Sequence[str], captions_per_image: Sequence[Sequence[str]]) -> List[Dict[int, float]]:
    """One log line per image: Div-1 / Div-2 over that image's samples (what sampled winners exist to move)."""
    out = []
    for name, caps in zip(img_name, captions_per_image):
        d = distinct_n(caps)
        logger.info(f"diversity of {len(caps)} samples of {name}: Div-1 {d[1]:.3f}, Div-2 {d[2]:.3f}")
        out.append(d)
    return out
