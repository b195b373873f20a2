"""The YouTube encoder (csrc/yt_encode.hip) vs the CPU oracle on every
adversarial corpus of tests/_corpora.py (``yt_*``).

Each run pre-fills the output with 0xA5 and puts it between two 256-byte
guard regions: a line the write pass leaves a hole in cannot inherit
stale correct bytes, a write outside the buffer is seen, and
``line_len`` (the measure pass) must equal the oracle's lengths, so the
two passes cannot disagree unnoticed. No corpus string holds byte 0xA5
(test_corpora_preconditions pins that), so none may survive in ``out``.
"""
import numpy as np
import pytest
import torch

from crawler_amd.youtube.batch import (build_corpus, build_corpus_device,
                                       build_corpus_fast, encode_yt_batch)
from crawler_amd.youtube.synth import SyntheticYouTubeIndex

import _corpora as C

pytestmark = pytest.mark.gpu

POISON = C.YT_POISON
GUARD = 256
CORPORA = (["url", "sanitize", "numbers"]
           + ["esc%d" % j for j in range(6)]
           + ["shape%d" % n for n in C.YT_SHAPE_NS])


@pytest.fixture(scope="module")
def gpu_mod():
    from crawler_amd.ops import gpu

    gpu.require_lib()
    return gpu


_batches = {}
_oracles = {}


def _batch(name):
    """Named corpus, built once per session and never mutated."""
    if not _batches:
        _batches.update(C.yt_corpora())
        assert sorted(_batches) == sorted(CORPORA)
    return _batches[name]


def _oracle(key, batch, now=C.NOW):
    if key not in _oracles:
        _oracles[key] = encode_yt_batch(batch, now=now)
    return _oracles[key]


def _run(gpu_mod, batch, now=C.NOW, grid=0):
    res = gpu_mod.yt_parse_encode(batch.to("cuda:0"), now=now, grid=grid,
                                  _poison=POISON, _guard=GUARD)
    torch.cuda.synchronize()
    return res


def _check(res, lines, what):
    out_t, line_off, line_len = res          # still unpacks as a triple
    want_len = np.array([len(l) for l in lines], dtype=np.int64)
    want_off = np.concatenate([[0], np.cumsum(want_len)[:-1]]) \
        if len(lines) else np.zeros(0, dtype=np.int64)
    lens = line_len.cpu().numpy()
    offs = line_off.cpu().numpy()
    assert lens.dtype == np.int32 and offs.dtype == np.int64
    raw = res.raw.cpu().numpy()
    total = raw.size - 2 * GUARD
    assert out_t.numel() == total
    out = bytes(raw[GUARD:GUARD + total])
    assert out == bytes(out_t.cpu().numpy())
    # guards first: with a write outside the buffer nothing else counts
    assert (raw[:GUARD] == POISON).all(), f"{what}: write before the buffer"
    assert (raw[GUARD + total:] == POISON).all(), \
        f"{what}: write past the buffer"
    # line_off is the exclusive prefix sum of the measured lengths
    assert offs.tolist() == (np.cumsum(lens.astype(np.int64))
                             - lens).tolist()
    for i, gl in enumerate(lines):
        dev = out[offs[i]: offs[i] + lens[i]]
        assert dev == gl, (
            f"{what} line {i} (measured {lens[i]}, oracle {len(gl)}):\n"
            f"GPU: {_around(dev, gl)!r}\nCPU: {_around(gl, dev)!r}")
    assert lens.tolist() == want_len.tolist()
    assert offs.tolist() == want_off.tolist()
    assert out == b"".join(lines)
    assert POISON not in out, f"{what}: unwritten byte inside a line"


def _around(a, b):
    """``a`` from 60 bytes before its first difference with ``b``."""
    k = next((j for j, (x, y) in enumerate(zip(a, b)) if x != y),
             min(len(a), len(b)))
    return a[max(0, k - 60): k + 240]


@pytest.mark.parametrize("grid", [0, 1, 2])
@pytest.mark.parametrize("corpus", CORPORA)
def test_yt_corpus(gpu_mod, corpus, grid):
    """Byte-exact at the default grid and with one and two blocks (each
    wave then walks several rows in the grid-stride loop; with n % 4 != 0
    some waves of the last block get no row)."""
    batch = _batch(corpus)
    res = _run(gpu_mod, batch, grid=grid)
    _check(res, _oracle(corpus, batch), f"{corpus} grid={grid}")


@pytest.mark.parametrize("micro", [0, 890000, 5])
def test_yt_capture_time_lengths(gpu_mod, micro):
    """capture_time is RFC3339Nano: its length changes with ``now``'s
    fraction (none, .89, .000005) while created_at stays at seconds."""
    now = C.NOW.replace(microsecond=micro)
    batch = _batch("shape9")
    lines = _oracle(("shape9", micro), batch, now=now)
    _check(_run(gpu_mod, batch, now=now), lines, f"micro={micro}")


def test_yt_empty_batch(gpu_mod):
    """n = 0 launches nothing and returns empty tensors of the right
    dtypes, with and without the seams."""
    from crawler_amd.youtube.batch import pack_videos

    batch = pack_videos([], [], [])
    assert encode_yt_batch(batch, now=C.NOW) == []
    res = _run(gpu_mod, batch)
    _check(res, [], "empty")
    out, line_off, line_len = gpu_mod.yt_parse_encode(batch.to("cuda:0"),
                                                      now=C.NOW)
    torch.cuda.synchronize()
    assert out.numel() == 0 and out.dtype == torch.uint8
    assert tuple(line_off.shape) == (0,) and line_off.dtype == torch.int64
    assert tuple(line_len.shape) == (0,) and line_len.dtype == torch.int32
    assert out.device.type == "cuda"


def test_yt_seams_off_same_bytes(gpu_mod):
    """Without the seams the result is the same triple, with no raw."""
    batch = _batch("url")
    res = gpu_mod.yt_parse_encode(batch.to("cuda:0"), now=C.NOW)
    torch.cuda.synchronize()
    out, line_off, line_len = res
    assert res.raw is None
    assert bytes(out.cpu().numpy()) == b"".join(_oracle("url", batch))


WRAP = 26 ** 5


@pytest.mark.parametrize("universe", [1, 61, 63])
@pytest.mark.parametrize("i0", [1000, WRAP - 32])
def test_device_corpus_from_i0(gpu_mod, universe, i0):
    """build_corpus_device(i0=...) rows encode line for line like the
    host builders' rows i0..i0+63 (channel tables differ in order, the
    lines must not). 26**5 - 32 crosses the prefix wrap; a universe of 1
    puts every row on one channel."""
    n = 64
    idx = SyntheticYouTubeIndex(seed=17, universe_channels=universe)
    if i0 == 1000:
        want = encode_yt_batch(build_corpus_fast(idx, i0 + n,
                                                 crawl_label="dev"),
                               now=C.NOW)[i0:]
    else:
        want = encode_yt_batch(build_corpus(idx, n, crawl_label="dev",
                                            i0=i0), now=C.NOW)
    assert len(want) == n
    dev = build_corpus_device(
        SyntheticYouTubeIndex(seed=17, universe_channels=universe), n,
        "cuda:0", crawl_label="dev", i0=i0)
    torch.cuda.synchronize()
    if universe == 1:
        assert dev.n_channels == 1
    # the device rows through the host oracle ...
    assert encode_yt_batch(dev.to("cpu"), now=C.NOW) == want
    # ... and through the device encoder
    _check(_run(gpu_mod, dev), want, f"device i0={i0} u={universe}")


def _walk_ids(idx, i0, n):
    """build_corpus's walk: base-26 prefix of i, video_id(prefix, i % 7)."""
    import string

    ids = []
    for i in range(i0, i0 + n):
        p, v = "", i
        for _ in range(5):
            p = string.ascii_lowercase[v % 26] + p
            v //= 26
        ids.append(idx.video_id(p, i % 7))
    return ids


@pytest.mark.parametrize("i0,n", [(0, 1), (0, 257), (WRAP - 32, 64),
                                  (123_456_789, 3)])
def test_ids_from_index_device(gpu_mod, i0, n):
    """The id kernel against the Python walk: one id, one thread past a
    full block, across the 26**5 wrap, and an i0 far past it."""
    from crawler_amd.youtube.batch import yt_ids_from_index_device

    idx = SyntheticYouTubeIndex(seed=17, universe_channels=63)
    ids = yt_ids_from_index_device(idx, i0, n, "cuda:0")
    torch.cuda.synchronize()
    assert tuple(ids.shape) == (n, 11) and ids.dtype == torch.uint8
    got = [bytes(r).decode() for r in ids.cpu().numpy()]
    assert got == _walk_ids(idx, i0, n)


def test_ids_from_index_device_empty(gpu_mod):
    from crawler_amd.youtube.batch import yt_ids_from_index_device

    idx = SyntheticYouTubeIndex(seed=17, universe_channels=63)
    ids = yt_ids_from_index_device(idx, 5, 0, "cuda:0")
    assert tuple(ids.shape) == (0, 11) and ids.dtype == torch.uint8
    assert ids.device.type == "cuda"


def test_device_corpus_empty(gpu_mod):
    """Zero videos: an empty batch, through the oracle and the encoder."""
    idx = SyntheticYouTubeIndex(seed=17, universe_channels=63)
    b = build_corpus_device(idx, 0, "cuda:0")
    torch.cuda.synchronize()
    assert b.n == 0 and b.n_channels == 0
    assert encode_yt_batch(b.to("cpu")) == []
    out, line_off, line_len = gpu_mod.yt_parse_encode(b)
    torch.cuda.synchronize()
    assert out.numel() == 0 and line_len.numel() == 0
