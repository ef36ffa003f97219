"""Seeds and draw records for czc_generate_rows_draw (include/conzic_hip.h): host-side helpers, the counterpart of signals.py.

A row of a czc_generate_rows_draw call may draw its winner from softmax_K(final_score / tau) with a counter-based generator
(Philox4x32-10) keyed by a 64-bit seed of the row's own.  The seed is what makes sample s of image i reproducible whatever batch,
stream or replica the row lands in, so it is derived from the run's seed, a key of the image and the sample's index alone."""
import zlib
from typing import List, Optional, Sequence, Union

from . import native

_M64 = (1 << 64) - 1


def splitmix64(x: int) -> int:
    """One output of the splitmix64 generator (Steele, Lea, Flood 2014) for state `x`: x += 0x9E3779B97F4A7C15, then the
    finaliser z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31 (all mod 2^64)."""
    z = (int(x) + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def image_key(name: Union[str, int]) -> int:
    """A 64-bit key of an image: an integer as it is, a name (its file name, say) through CRC-32 of its UTF-8 bytes -- stable
    across processes, unlike hash()."""
    if isinstance(name, int):
        return name & _M64
    return zlib.crc32(str(name).encode("utf8")) & 0xffffffff


def row_seed(base_seed: int, image_key: int, sample_index: int, extra: int = 0) -> int:
    """The seed of (image, sample) under a run's `base_seed`: a chain of splitmix64 mixes,
        h = splitmix64(base_seed); h = splitmix64(h ^ image_key); h = splitmix64(h ^ sample_index); h = splitmix64(h ^ extra)
    with every operand reduced mod 2^64.  `extra` tells apart rows that share image and sample (a length or signal column)."""
    h = splitmix64(int(base_seed) & _M64)
    for v in (image_key, sample_index, extra):
        h = splitmix64(h ^ (int(v) & _M64))
    return h


def make_draw(seed: int, tau: float, step0: int = 0) -> native.Draw:
    tau = float(tau)
    if not (tau >= 0.0) or tau == float("inf"):
        raise ValueError(f"tau = {tau!r} must be finite and >= 0")
    if not 0 <= int(step0) < (1 << 32):
        raise ValueError(f"step0 = {step0!r} outside [0, 2^32)")
    return native.Draw(int(seed) & _M64, tau, int(step0))


def draw_rows(seeds: Sequence[int], tau: Union[float, Sequence[float]], step0: int = 0) -> List[native.Draw]:
    """The [R] draw records of a call: row r gets seeds[r], tau (one value or one per row) and the call's step offset."""
    seeds = list(seeds)
    taus = [float(tau)] * len(seeds) if isinstance(tau, (int, float)) else [float(t) for t in tau]
    if len(taus) != len(seeds):
        raise ValueError(f"{len(taus)} taus for {len(seeds)} seeds")
    return [make_draw(s, t, step0) for s, t in zip(seeds, taus)]


def sample_rows(base_seed: int, image_keys: Sequence[int], samples: int, tau: float, columns: int = 1, step0: int = 0,
                sample0: int = 0, column0: int = 0) -> Optional[List[native.Draw]]:
    """Draw records in the row order of the runtime's batched calls: row (c * samples + s) * B + b = column column0 + c (a length
    or signal column; one for a plain samples call), sample sample0 + s, image b of `image_keys`.  The seed of a row is
    row_seed(base_seed, image key, sample, column): a serial loop that runs sample s alone (samples = 1, sample0 = s) gives the
    row the seed the batched call gives it.  tau == 0: None (no row draws)."""
    if not tau:
        return None
    return [make_draw(row_seed(base_seed, k, sample0 + s, column0 + c), tau, step0)
            for c in range(int(columns)) for s in range(int(samples)) for k in image_keys]


def describe(draws: Optional[Sequence[native.Draw]]) -> str:
    """What a log line says about the rows it covers: `` sample_tau T seeds [0x...]`` (empty when no row draws)."""
    if not draws:
        return ""
    return f" sample_tau {draws[0].tau:g} seeds [{', '.join(hex(d.seed) for d in draws)}]"
