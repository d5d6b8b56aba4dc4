"""The model of the string dictionary (include/aqg.h: aqg_str_encode, aqg_str_encode_sharded, aqg_str_encode_last), in plain Python.

The contract: astring_view keys compare by the CONTENT of their NUL-terminated strings; a NULL row pointer is the empty string; the
code of a row is the dense id of its content in first-occurrence order; over row-range shards there is ONE dictionary in GLOBAL
first-occurrence order (the shards concatenated in rank order).  codes() and codes_sharded() state that and know nothing of the library.

hash64(), with_hash() and collision() are WHITE-BOX ON PURPOSE: hash64 is a bit-exact model of str_hash_kernel
(aquery2_amd/csrc/strdict.hip), and the other two invert it to make strings with a chosen hash and pairs of different strings under
one hash -- the only way to reach the verify kernel's mismatch and the host fallback behind it, whose natural rate is ~n^2 / 2^65.
Whoever changes the kernel's hash changes this model in the same commit; tests/test_gpu_strdict.py notices when the two part, because
its collision cases then report the DEVICE route where they expect FALLBACK.  tests/test_strdict_model.py holds codes() to the oracle."""
import numpy as np

MASK = (1 << 64) - 1
SEED = 0x9E3779B97F4A7C15                      # str_hash_kernel: h = SEED ^ length
MUL = 0xD6E8FEB86659FD93                       # str_hash_kernel: the multiplier of every word step and of the final step (odd)
MUL_INV = pow(MUL, -1, 1 << 64)
ROUTE_HOST, ROUTE_DEVICE, ROUTE_FALLBACK = 1, 2, 4          # AQG_STR_ROUTE_*
DEVICE_MIN = 1 << 16                           # rows from which aqg_str_encode builds the dictionary on the device


def content(s):
    """what a row pointer stands for: None (NULL) is the empty string; a C string holds no NUL"""
    s = b"" if s is None else bytes(s)
    assert 0 not in s, "a NUL-terminated string cannot hold a NUL"
    return s


def codes(strs):
    """(codes uint32[n], ndistinct, first_rows uint32[ndistinct]): dense ids by content in first-occurrence order"""
    ids, first = {}, []
    out = np.empty(len(strs), np.uint32)
    for i, s in enumerate(strs):
        s = content(s)
        c = ids.get(s)
        if c is None:
            c = ids[s] = len(ids)
            first.append(i)
        out[i] = c
    return out, len(ids), np.array(first, dtype=np.uint32)


def codes_sharded(shards):
    """(per-rank code arrays, global ndistinct): ONE dictionary over the shards concatenated in rank order, split back per rank"""
    c, nd, _ = codes([s for sh in shards for s in sh])
    cuts = np.cumsum([0] + [len(sh) for sh in shards])
    return [c[cuts[r]:cuts[r + 1]] for r in range(len(shards))], nd


def expected_route(n, collides):
    """(route, mismatch flag) of aqg_str_encode_last for n rows; collides: the column holds two different strings under one hash and length"""
    if n < DEVICE_MIN:
        return ROUTE_HOST, 0
    return (ROUTE_FALLBACK, 1) if collides else (ROUTE_DEVICE, 0)


# ---- the hash of str_hash_kernel and its inverse --------------------------------------------------------------------------------------
def _step(h, w):
    """one 8-byte word: h = (h ^ w) * MUL; h ^= h >> 32"""
    h = ((h ^ w) * MUL) & MASK
    return h ^ (h >> 32)


def _final(h):
    h = (h * MUL) & MASK
    return h ^ (h >> 29)


def hash64(b):
    """str_hash_kernel's 64 bits of the bytes b: seed ^ length, a multiply-xorshift step per little-endian 8-byte word (the tail word
    zero-padded), a final multiply and a xorshift by 29"""
    b = bytes(b)
    h = SEED ^ len(b)
    for p in range(0, len(b), 8):
        h = _step(h, int.from_bytes(b[p:p + 8], "little"))
    return _final(h)


def _unstep(h):
    """h ^ w of the step whose result is h (x ^ x >> 32 is its own inverse; MUL is odd)"""
    h ^= h >> 32
    return (h * MUL_INV) & MASK


def _unfinal(y):
    x = y ^ (y >> 29) ^ (y >> 58)              # the inverse of x ^ x >> 29 on 64 bits
    return (x * MUL_INV) & MASK


def _word(rng):
    """8 random bytes, none of them NUL, as a little-endian word"""
    return int.from_bytes(bytes(rng.integers(1, 256, 8, dtype=np.uint8)), "little")


def _nul_free(w):
    return all((w >> (8 * k)) & 0xFF for k in range(8))


def with_hash(target, rng):
    """a 16-byte NUL-free string whose hash64 is `target`: a random first word, the second solved for (every step is a bijection on 64
    bits), again while the second holds a zero byte (about 3 % of the tries)"""
    want = _unstep(_unfinal(target & MASK))    # state after the first word ^ the second word
    while True:
        w1 = _word(rng)
        w2 = _step(SEED ^ 16, w1) ^ want
        if _nul_free(w2):
            s = w1.to_bytes(8, "little") + w2.to_bytes(8, "little")
            assert hash64(s) == target & MASK
            return s


def collision(rng, prefix=b""):
    """two different NUL-free strings of 16 bytes with equal hash64: first words a1 != b1 and a2 chosen, b2 = a2 ^ state(a1) ^ state(b1).
    prefix: whole NUL-free words that both strings start with (the pair then differs in its last 16 bytes only: a comparison that
    stops early takes the two for one)"""
    assert len(prefix) % 8 == 0 and 0 not in prefix
    h0 = SEED ^ (len(prefix) + 16)
    for p in range(0, len(prefix), 8):
        h0 = _step(h0, int.from_bytes(prefix[p:p + 8], "little"))
    while True:
        a1, b1, a2 = _word(rng), _word(rng), _word(rng)
        b2 = a2 ^ _step(h0, a1) ^ _step(h0, b1)
        if a1 != b1 and _nul_free(b2):
            a = prefix + a1.to_bytes(8, "little") + a2.to_bytes(8, "little")
            b = prefix + b1.to_bytes(8, "little") + b2.to_bytes(8, "little")
            assert a != b and hash64(a) == hash64(b)
            return a, b


def ordinary16(rng, avoid, prefix=b""):
    """prefix + 16 NUL-free bytes whose hash is none of the hashes of `avoid`: the control that stands in for a colliding partner"""
    taken = {hash64(s) for s in avoid}
    while True:
        s = prefix + bytes(rng.integers(1, 256, 16, dtype=np.uint8))
        if hash64(s) not in taken:
            return s
