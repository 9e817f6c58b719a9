"""The words a sharded CEM step all-reduces (``include/l2a.h``: ``l2a_cem_shard_pack`` / ``_unpack``, ``l2a_cem_word_encode`` /
``_decode``), without a GPU: the entry points are declared and bound, the host helpers keep every bit of a return, and a NumPy
model of the gather - built from those helpers and ``MPCController._shard_range``, pushed through the loopback world's MAX
all-reduce - returns the concatenated shards bit for bit, with the flag and the digest pair behind them."""

import ctypes
import os
import re

import numpy as np
import pytest

from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.policies.mpc_controller import MPCController
from loopback_world import LoopbackWorld

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIGEST_MASK = 0x7FFFFFFFFFFF

NEW_SYMBOLS = {
    "l2a_cem_shard_pack": ("int", 9),
    "l2a_cem_shard_unpack": ("int", 7),
    "l2a_cem_word_encode": ("unsigned long long", 1),
    "l2a_cem_word_decode": ("int", 2),
    "l2a_cem_controller_create_sharded_device": ("int", 18),
}


def test_sharded_cem_entry_points_are_declared_listed_and_bound():
    text = open(os.path.join(ROOT, "include", "l2a.h")).read()
    lib = _lib.load()
    for name, (ret, arity) in NEW_SYMBOLS.items():
        found = re.search(r"^%s %s\(([^;]*)\);" % (re.escape(ret), name), text, re.M)
        assert found, "%s is not declared in include/l2a.h" % name
        assert len(found.group(1).split(",")) == arity, name           # the header's own parameter count
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert len(getattr(lib, name).argtypes) == arity, name
    assert lib.l2a_cem_word_encode.restype is ctypes.c_ulonglong
    assert int(re.search(r"#define L2A_DIGEST_MASK (0x[0-9a-f]+)ull", text).group(1), 16) == DIGEST_MASK


def _encode(lib, bits):
    """``l2a_cem_word_encode`` of the float with these bits."""
    value = ctypes.c_float.from_buffer_copy(np.array([bits], dtype=np.uint32).tobytes())       # (no float conversion on the way)
    return int(lib.l2a_cem_word_encode(value))


def _decode(lib, word):
    out = ctypes.c_float()
    present = lib.l2a_cem_word_decode(ctypes.c_ulonglong(int(word)), ctypes.byref(out))
    return present, ctypes.c_uint32.from_buffer(out).value


# NaNs (quiet, with payloads, negative), +-0.0, +-inf, denormals, ordinary values.  (Signalling NaNs are left out: passing one
# BY VALUE through the C calling convention may quiet it on the way, before the library sees it; the kernels move words, not floats.)
SPECIAL_BITS = [0x7FC00000, 0x7FC00001, 0x7FD12345, 0xFFC00000, 0xFFFFFFFF, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000,
                0x00000001, 0x807FFFFF, 0x00400000, 0x3F800000, 0xBF800000, 0x42F6E979, 0xC47A0000, 0x7F7FFFFF, 0xFF7FFFFF]


def test_word_encode_decode_round_trip_keeps_every_bit():
    lib = _lib.load()
    rs = np.random.RandomState(11)
    ordinary = rs.randn(64).astype(np.float32).view(np.uint32).tolist()
    for bits in SPECIAL_BITS + ordinary:
        word = _encode(lib, bits)
        assert 0 < word < 2 ** 63, hex(bits)
        assert word == (1 << 32) | bits, hex(bits)
        assert _decode(lib, word) == (1, bits), hex(bits)
    assert _decode(lib, 0) == (0, 0)                                    # absent: decoded as 0.0f
    assert lib.l2a_cem_word_decode(ctypes.c_ulonglong(0), None) == 0    # (the value is optional)


def _table(m, n, seed):
    """An [m, n] fp32 returns table with non-finite and signed-zero entries among ordinary ones."""
    rs = np.random.RandomState(seed)
    bits = (rs.randn(m, n) * 100.0).astype(np.float32).view(np.uint32)
    flat = bits.reshape(-1)
    for k, special in enumerate(SPECIAL_BITS):
        flat[(7 * k + seed) % flat.size] = special
    return bits


def _rank_words(lib, bits, rank, world, flag, digest):
    """What `rank` contributes: m * n + 3 int64 words (the model of ``l2a_cem_shard_pack``)."""
    m, n = bits.shape
    lo, hi = MPCController._shard_range(n, rank, world)
    words = np.zeros((m * n + 3,), dtype=np.int64)
    for i in range(m):
        for j in range(lo, hi):
            words[i * n + j] = _encode(lib, int(bits[i, j]))
    d = digest & DIGEST_MASK
    words[m * n:] = [1 if flag else 0, d, DIGEST_MASK - d]
    return words, (lo, hi)


def _decode_table(lib, words, m, n):
    """The model of ``l2a_cem_shard_unpack``: ``(table bits [m, n], verdict [flag, holes, digest mismatch])``."""
    out = np.zeros((m, n), dtype=np.uint32)
    holes = 0
    for e in range(m * n):
        present, value = _decode(lib, int(words[e]))
        holes += 0 if present else 1
        out[e // n, e % n] = value
    tail = [int(w) for w in words[m * n:]]
    return out, [1 if tail[0] else 0, holes, 0 if tail[1] + tail[2] == DIGEST_MASK else 1]


@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("world_size", [1, 2, 3, 8, "n + 3"])
def test_the_max_reduce_of_the_words_is_the_gather_of_the_shards(world_size, m):
    lib = _lib.load()
    n = 13
    world_size = n + 3 if world_size == "n + 3" else world_size
    bits = _table(m, n, 3 + m)
    shards = {}

    def program(rank, comm):
        words, shards[rank] = _rank_words(lib, bits, rank, world_size, flag=False, digest=0x1234567890ABCDEF)
        assert np.all(words >= 0) and np.all(words[:m * n] < 2 ** 33)   # signed MAX is the unsigned one
        return comm.reduce_max(words)

    world = LoopbackWorld(world_size)
    outs = world.run(program)
    assert world.passes == 2 and world.calls == [1] * world_size
    widths = [hi - lo for lo, hi in (shards[r] for r in range(world_size))]
    assert sum(widths) == n and max(widths) - min(widths) <= 1
    if world_size in (3, 8):
        assert len(set(widths)) == 2                                    # uneven shards
    if world_size > n:
        assert widths.count(0) == 3                                     # more ranks than candidates: empty shards
    # the reduced table = the shards side by side, bit for bit, on every rank; nobody flagged, the digests agree
    parts = world.collectives[0]["parts"]
    for rank, reduced in enumerate(outs):
        got, verdict = _decode_table(lib, reduced, m, n)
        assert got.tobytes() == bits.tobytes(), rank
        assert verdict == [0, 0, 0], rank
    for rank in range(world_size):
        lo, hi = shards[rank]
        mine = parts[rank][:m * n].reshape(m, n)
        assert np.count_nonzero(mine) == m * (hi - lo) and not mine[:, :lo].any() and not mine[:, hi:].any()


def test_flag_digest_and_holes_in_the_reduced_words():
    lib = _lib.load()
    m, n, world_size = 2, 13, 3
    bits = _table(m, n, 9)

    def run(flagged=None, odd_digest=None, missing=None):
        def program(rank, comm):
            words, _ = _rank_words(lib, bits, rank, world_size, flag=(rank == flagged), digest=77 if rank == odd_digest else 42)
            if rank == missing:
                words[:m * n] = 0                                       # a rank whose returns never arrive
            return comm.reduce_max(words)
        outs = LoopbackWorld(world_size).run(program)
        assert all(np.array_equal(o, outs[0]) for o in outs)            # every rank holds the same reduced words
        return _decode_table(lib, outs[0], m, n)

    assert run()[1] == [0, 0, 0]
    got, verdict = run(flagged=1)
    assert verdict == [1, 0, 0] and got.tobytes() == bits.tobytes()     # any rank's flag reaches every rank
    assert run(odd_digest=2)[1] == [0, 0, 1]                            # one rank built differently: the pair no longer adds up
    lo, hi = MPCController._shard_range(n, 1, world_size)
    got, verdict = run(missing=1)
    assert verdict == [0, m * (hi - lo), 0]                             # a missing part: holes = exactly its width
    assert not got[:, lo:hi].any() and got[:, :lo].tobytes() == bits[:, :lo].tobytes()
