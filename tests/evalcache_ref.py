"""The evaluation cache's table (csrc/evalcache.hip, include/zeroclone.h "evaluation cache") in
plain integer arithmetic: the key hash and the bits taken from it, the block's byte layout, a
model of the table under flushes of ONE ROW EACH — where what the kernels do is fully determined
— and deterministic finders of the keys the GPU tests need: keys that differ in one word and
share set and tag, and keys whose raw tag is 0 or 1.

tests/test_gpu_eval_cache_keys.py holds the device to this file (its first test compares the
placement of 256 keys), so a change of the hash changes this file in the same commit.  No GPU
and no library: numpy alone."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

WAYS = 8
HEADER_BYTES = 64
M1, M2 = np.uint64(0xff51afd7ed558ccd), np.uint64(0xc4ceb9fe1a85ec53)
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
S33 = np.uint64(33)


def mix64(x):
    """The murmur3 finaliser on a uint64 array (arithmetic modulo 2^64)."""
    x = np.array(x, dtype=np.uint64, copy=True)
    with np.errstate(over="ignore"):
        x ^= x >> S33
        x *= M1
        x ^= x >> S33
        x *= M2
        x ^= x >> S33
    return x


def _mixed_words(keys):
    """[n, kw] -> every word mixed with its position, [n, kw]."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    with np.errstate(over="ignore"):
        salt = GOLDEN * np.arange(1, keys.shape[1] + 1, dtype=np.uint64)
        return mix64(keys + salt[None, :])


def key_hash(keys):
    """keys [n, kw] uint64 -> the table's hash [n] uint64: word i mixed as mix64(word + GOLDEN *
    (i + 1)), the results xor-ed, the xor mixed again."""
    keys = np.asarray(keys, dtype=np.uint64)
    if keys.ndim == 1:
        keys = keys[None, :]
    return mix64(np.bitwise_xor.reduce(_mixed_words(keys), axis=1))


def tag(h):
    """The 16-bit tag of a meta word: the hash's top 16 bits, 0 remapped to 1 (0 is "empty")."""
    t = (np.asarray(h, dtype=np.uint64) >> np.uint64(48)).astype(np.uint32)
    return np.where(t == 0, np.uint32(1), t)


def raw_tag(h):
    return (np.asarray(h, dtype=np.uint64) >> np.uint64(48)).astype(np.uint32)


def set_index(h, sets):
    return ((np.asarray(h, dtype=np.uint64) & np.uint64(0xFFFFFFFF)) & np.uint64(sets - 1)).astype(np.int64)


def victim_way(h):
    """The way of a full set that a commit replaces."""
    return ((np.asarray(h, dtype=np.uint64) >> np.uint64(32)) & np.uint64(WAYS - 1)).astype(np.int64)


def claim_start(h, mask):
    """The merged probe's first claim slot (mask = the claim table's slots - 1)."""
    return ((np.asarray(h, dtype=np.uint64) >> np.uint64(24)) & np.uint64(mask)).astype(np.int64)


Layout = namedtuple("Layout", "sets entries epoch meta keys values logits lstride bytes")


def layout(entries, key_bytes, logit_bytes):
    """Byte offsets into the table's block:
        [header 64 B: epoch u32][meta u32 x E][keys key_bytes x E][values f64 x E][logits lstride x E]
    sets = the largest power of two with 8 * sets <= entries, E = 8 * sets, lstride = logit_bytes
    rounded up to 16."""
    assert entries >= 1 and key_bytes >= 8 and key_bytes % 8 == 0 and key_bytes <= 512 and logit_bytes % 2 == 0
    sets = 1
    while sets * 2 * WAYS <= entries:
        sets *= 2
    E = sets * WAYS
    lstride = (logit_bytes + 15) & ~15
    meta = HEADER_BYTES
    keys = meta + 4 * E
    values = keys + key_bytes * E
    logits = values + 8 * E
    return Layout(sets, E, 0, meta, keys, values, logits, lstride, logits + lstride * E)


class TableModel:
    """The table under flushes of one row each (probe, then a commit launch).

    probe(key): the entry of the set's first way whose tag AND whole key equal the key's, else -1.
    commit(key, payload): dropped when a way of the set carries the key's tag; else the first
    empty way, else victim_way(h) — and dropped too when that way's epoch half equals the running
    epoch's (the kernel cannot tell such an entry from one claimed in this launch: only a full
    set whose victim is exactly 65536 commit launches old meets this).  The entry gets
    tag << 16 | (epoch & 0xFFFF).  Every commit launch, with or without a row, moves the epoch
    on by one.  `payload` is any Python object; the model keeps it per entry."""

    def __init__(self, entries, key_bytes, logit_bytes=0, epoch=0):
        self.lay = layout(entries, key_bytes, logit_bytes)
        self.kw = key_bytes // 8
        E = self.lay.entries
        self.meta = np.zeros(E, np.uint32)
        self.keys = np.zeros((E, self.kw), np.uint64)
        self.payload = [None] * E
        self.epoch = int(epoch)
        self.stats = {"probed": 0, "hits": 0, "inserts": 0, "dropped": 0}

    def _where(self, key):
        key = np.asarray(key, dtype=np.uint64).reshape(1, self.kw)
        h = key_hash(key)
        return key[0], h[0], int(set_index(h, self.lay.sets)[0]) * WAYS, int(tag(h)[0])

    def probe(self, key):
        key, _, e0, t = self._where(key)
        self.stats["probed"] += 1
        for w in range(WAYS):
            if int(self.meta[e0 + w]) >> 16 == t and np.array_equal(self.keys[e0 + w], key):
                self.stats["hits"] += 1
                return e0 + w
        return -1

    def commit(self, key=None, payload=None):
        """One commit launch: of `key` (a row that missed) or of no row (key None).  Returns the
        entry written, or -1."""
        entry = -1
        if key is not None:
            key, h, e0, t = self._where(key)
            ways = [int(m) for m in self.meta[e0:e0 + WAYS]]
            ep = self.epoch & 0xFFFF
            if not any(m >> 16 == t for m in ways):
                w = ways.index(0) if 0 in ways else int(victim_way(h))
                if not (ways[w] and (ways[w] & 0xFFFF) == ep):
                    entry = e0 + w
                    self.meta[entry] = (t << 16) | ep
                    self.keys[entry] = key
                    self.payload[entry] = payload
            self.stats["inserts" if entry >= 0 else "dropped"] += 1
        self.epoch = (self.epoch + 1) & 0xFFFFFFFF
        return entry

    def flush(self, key, payload):
        """-> (the entry hit or -1, the entry written or -1)."""
        hit = self.probe(key)
        return hit, self.commit(None if hit >= 0 else key, payload)

    def used_entries(self):
        return int((self.meta != 0).sum())


# ---------------------------------------------------------------------------------------------
# finders: deterministic (fixed seeds), cached

DRAW = 40000           # candidates a round of colliding_pairs draws
MAX_ROUNDS = 64        # its cap: 2.56 M candidates
TAG_DRAW = 400000      # candidates a round of key_with_raw_tag draws
TAG_MAX_ROUNDS = 256   # its cap: 102.4 M candidates (a hit takes 65536 * sets draws on average)


def _base(kw, seed):
    return np.random.default_rng(seed).integers(0, 1 << 64, kw, dtype=np.uint64)


def _variants(base, j, words):
    """The hashes of `base` with word j replaced by each of `words` (two mixes a candidate,
    whatever the key's length)."""
    kw = base.shape[0]
    rest = np.bitwise_xor.reduce(np.delete(_mixed_words(base[None, :])[0], j)) if kw > 1 else np.uint64(0)
    with np.errstate(over="ignore"):
        return mix64(mix64(words + GOLDEN * np.uint64(j + 1)) ^ rest)


@functools.lru_cache(maxsize=None)
def _colliding_groups(kw, j, sets, n, size):
    base = _base(kw, 1000 * kw + j)
    rng = np.random.default_rng(77000 + 1000 * kw + 10 * j + (sets > 1))
    words = np.zeros(0, np.uint64)
    for _ in range(MAX_ROUNDS):
        words = np.unique(np.concatenate([words, rng.integers(0, 1 << 64, DRAW, dtype=np.uint64)]))
        h = _variants(base, j, words)
        group = set_index(h, sets) << 16 | tag(h).astype(np.int64)
        order = np.argsort(group, kind="stable")
        g = group[order]
        starts, end = [], 0                               # runs of `size` candidates of one set and tag,
        for s in np.flatnonzero(g[size - 1:] == g[:len(g) - size + 1]):   # disjoint: no key twice
            if s >= end:
                starts.append(int(s))
                end = s + size
                if len(starts) == n:
                    break
        if len(starts) == n:
            out = np.tile(base, (n, size, 1))
            for k in range(size):
                out[:, k, j] = words[order[np.array(starts) + k]]
            return out
    raise RuntimeError(f"no {n} groups of {size} colliding keys for kw {kw}, word {j}, {sets} sets in "
                       f"{MAX_ROUNDS * DRAW} candidates")


def colliding_groups(kw, j, sets, n, size):
    """[n, size, kw] uint64: the `size` keys of a group differ from each other in word j only and
    share set (of `sets`) and tag; the n * size keys are pairwise distinct."""
    return _colliding_groups(int(kw), int(j), int(sets), int(n), int(size)).copy()


def colliding_pairs(kw, j, sets, n):
    """(A, B), each [n, kw] uint64: A[i] and B[i] differ in word j only and share set and tag."""
    g = colliding_groups(kw, j, sets, n, 2)
    return g[:, 0].copy(), g[:, 1].copy()


@functools.lru_cache(maxsize=None)
def _key_with_raw_tag(kw, t, sets, in_set):
    base = _base(kw, 5000 + kw)
    rng = np.random.default_rng(88000 + 100 * kw + t)
    for _ in range(TAG_MAX_ROUNDS):
        words = rng.integers(0, 1 << 64, TAG_DRAW, dtype=np.uint64)
        h = _variants(base, kw - 1, words)
        ok = raw_tag(h) == t
        if in_set is not None:
            ok &= set_index(h, sets) == in_set
        if ok.any():
            key = base.copy()
            key[kw - 1] = words[np.flatnonzero(ok)[0]]
            return key
    raise RuntimeError(f"no key of raw tag {t} for kw {kw} in {TAG_MAX_ROUNDS * TAG_DRAW} candidates")


def key_with_raw_tag(kw, t, sets=1, in_set=None):
    """A key [kw] uint64 whose hash has the top 16 bits == t (0: the tag the table remaps to 1),
    in set `in_set` of `sets` when that is given.  The finder keeps drawing, TAG_DRAW last words
    of one base key a round, until it has one: two or three of 400000 hashes have a given raw
    tag, and a round may have none."""
    return _key_with_raw_tag(int(kw), int(t), int(sets), None if in_set is None else int(in_set)).copy()


def raw_tag_pair(kw, sets):
    """(a key of raw tag 0, a key of raw tag 1) in one set of `sets`."""
    k0 = key_with_raw_tag(kw, 0)
    k1 = key_with_raw_tag(kw, 1, sets, int(set_index(key_hash(k0), sets)[0]))
    return k0, k1
