"""What the probe modules share: the placement word the kernels record, the
hashes of their host mirrors, and the pieces every per-wave summariser is
made of. Pure numpy, imported lazily; needs no GPU."""
from __future__ import annotations

_M32 = 0xFFFFFFFF
_M64 = (1 << 64) - 1

# keys of a decoded placement, in the order decode_hw_simd returns them
PLACE_KEYS = ("xcc", "se", "sh", "cu", "simd")


def decode_hw_word(word) -> tuple:
    """(XCC_ID<<16 | HW_ID) placement word -> (xcc, se, sh, cu)."""
    w = int(word)
    return (w >> 16, (w >> 13) & 0x7, (w >> 12) & 0x1, (w >> 8) & 0xF)


def decode_hw_simd(word) -> tuple:
    """(XCC_ID<<16 | HW_ID) placement word -> (xcc, se, sh, cu, simd), with
    SIMD_ID at HW_ID[5:4] as in the gfx9-family layout."""
    w = int(word)
    return decode_hw_word(w) + ((w >> 4) & 0x3,)


def _fmix32(h):
    """murmur3 32-bit finaliser on a numpy uint32 array."""
    import numpy as np

    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def _mix64(x):
    """splitmix64 finaliser on a numpy uint64 array (wraps mod 2^64)."""
    import numpy as np

    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _rotl32(x, k):
    import numpy as np

    return (x << np.uint32(k)) | (x >> np.uint32(32 - k))


def _u64_fields(rec, lo):
    """Fields [lo], [lo+1] of int32 records (lo word, hi word) as np.uint64."""
    import numpy as np

    low = (rec[..., lo].astype(np.int64) & 0xFFFFFFFF).astype(np.uint64)
    high = (rec[..., lo + 1].astype(np.int64) & 0xFFFFFFFF).astype(np.uint64)
    return (high << np.uint64(32)) | low


def units_seen(words, decode) -> int:
    """Distinct units (CUs or SIMDs, by `decode`) among placement words."""
    import numpy as np

    return len({decode(w) for w in np.unique(words)})


def checksum_outliers(checksums):
    """Which waves' checksum is not the majority's (all compute the same)."""
    import numpy as np

    values, counts = np.unique(checksums, return_counts=True)
    majority = values[counts.argmax()] if len(checksums) else 0
    return checksums != majority


class BadUnits:
    """Per bad unit (a decoded placement tuple): named counters, the earliest
    `first` tuple and OR-ed masks, rendered as the sorted list of dicts a
    summariser reports, placement keys first."""

    def __init__(self):
        self._units: dict = {}
    def add(self, place, counts: dict, first=None, masks: dict = None) -> None:
        """`first` is a tuple ordered by what came first; None reports none."""
        masks = masks or {}
        e = self._units.setdefault(place, {"counts": dict.fromkeys(counts, 0), "first": None,
                                           "masks": dict.fromkeys(masks, 0)})
        for key, value in counts.items():
            e["counts"][key] += int(value)
        if first is not None:
            e["first"] = first if e["first"] is None else min(e["first"], first)
        for key, value in masks.items():
            e["masks"][key] |= int(value)

    def entries(self, first_keys) -> list:
        """One dict per unit, sorted by placement: the placement, the counters,
        `first` under first_keys (-1 each when no wave gave one), the masks."""
        out = []
        for place in sorted(self._units):
            e = self._units[place]
            first = e["first"] if e["first"] is not None else (-1,) * len(first_keys)
            out.append({**dict(zip(PLACE_KEYS, place)), **e["counts"],
                        **dict(zip(first_keys, first)), **e["masks"]})
        return out


def place_keys(entries, width: int) -> set:
    """The placement tuples (width 4: CUs, 5: SIMDs) of a list of unit dicts."""
    return {tuple(e[k] for k in PLACE_KEYS[:width]) for e in entries}


def place_dicts(keys) -> list:
    """Placement tuples as sorted dicts: a union over several runs."""
    return [dict(zip(PLACE_KEYS, key)) for key in sorted(keys)]
