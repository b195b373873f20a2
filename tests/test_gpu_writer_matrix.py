"""Every JSONL writer variant vs the CPU oracle, on every hard corpus.

parse_encode has four writers (staged / plain / lds / scratch+compact).
Each run here selects one explicitly, asserts that it is the one that
ran (``res.writer``), and checks the output byte for byte against
golden_batch.encode_batch. Outputs are pre-filled with 0xA5 and sit
between two 256-byte guard regions, so a writer that skips bytes cannot
inherit stale correct ones from the allocator and a write outside the
buffer is seen."""
import numpy as np
import pytest
import torch

from crawler_amd.ops import batch as B
from crawler_amd.ops.golden_batch import encode_batch

import _corpora as C

pytestmark = pytest.mark.gpu

WRITERS = ["staged", "plain", "lds", "scratch"]
POISON = 0xA5
GUARD = 256


@pytest.fixture(scope="module")
def gpu_mod():
    from crawler_amd.ops import gpu

    gpu.require_lib()
    return gpu


_batches = {}
_oracles = {}


def _batch(name):
    """Named corpus, built once per session and never mutated."""
    if name not in _batches:
        if name.startswith("fuzz"):
            _batches[name] = C.fuzz_batch(int(name[4:]))
        elif name == "edges":
            _batches[name] = C.edge_batch()[1]
        elif name == "swar":
            _batches[name] = C.swar_batch()[1]
        elif name == "lds_ladder":
            _batches[name] = C.lds_ladder()
        elif name in ("stage_at", "stage_over"):
            from crawler_amd.ops import gpu

            at, over = C.stage_ladder(
                int(gpu.require_lib().crawl_stage_budget()),
                gpu._STAGE_FIXED)
            _batches["stage_at"], _batches["stage_over"] = at, over
        else:
            raise KeyError(name)
    return _batches[name]


def _oracle(key, batch, min_post_date=None):
    if key not in _oracles:
        _oracles[key] = encode_batch(batch, now=C.NOW,
                                     min_post_date=min_post_date)
    return _oracles[key]


def _select(monkeypatch, writer):
    """Environment + kwargs that ask parse_encode for ``writer``."""
    monkeypatch.delenv("CRAWL_NO_STAGED", raising=False)
    monkeypatch.delenv("CRAWL_LDS_WRITE", raising=False)
    if writer == "plain":
        monkeypatch.setenv("CRAWL_NO_STAGED", "1")
    elif writer == "lds":
        monkeypatch.setenv("CRAWL_LDS_WRITE", "1")
    return {"single_pass": writer == "scratch"}


def _run(gpu_mod, monkeypatch, writer, batch, **kw):
    kw.update(_select(monkeypatch, writer))
    res = gpu_mod.parse_encode(batch.to("cuda:0"), now=C.NOW,
                               _poison=POISON, _guard=GUARD, **kw)
    torch.cuda.synchronize()
    return res


def _check(gpu_mod, res, oracle, expect_writer):
    lines, links = oracle
    assert res.writer == expect_writer
    want_len = np.array([len(l) for l in lines], dtype=np.int64)
    want_off = np.concatenate([[0], np.cumsum(want_len)[:-1]]) \
        if len(lines) else np.zeros(0, dtype=np.int64)
    lens = res.line_len.cpu().numpy()
    offs = res.line_off.cpu().numpy()
    assert lens.dtype == np.int32 and offs.dtype == np.int64
    assert lens.tolist() == want_len.tolist()
    assert offs.tolist() == want_off.tolist()
    total = int(want_len.sum())
    assert res.out.numel() == total
    raw = res.raw.cpu().numpy()
    assert raw.size == total + 2 * GUARD
    out = bytes(raw[GUARD:GUARD + total])
    assert out == bytes(res.out.cpu().numpy())
    for i, gl in enumerate(lines):
        dev = out[offs[i]: offs[i] + lens[i]]
        assert dev == gl, (
            f"{expect_writer} line {i}:\nGPU: {dev[:300]!r}\n"
            f"CPU: {gl[:300]!r}")
    assert out == b"".join(lines)
    assert gpu_mod.links_to_python(res) == links
    assert (raw[:GUARD] == POISON).all(), "write before the buffer"
    assert (raw[GUARD + total:] == POISON).all(), "write past the buffer"


@pytest.mark.parametrize("corpus", ["fuzz11", "edges", "swar", "lds_ladder"])
@pytest.mark.parametrize("writer", WRITERS)
def test_writer_on_corpus(gpu_mod, monkeypatch, writer, corpus):
    batch = _batch(corpus)
    if corpus == "lds_ladder" and writer == "staged":
        # the ladder must reach the staged writer, not its fallback
        assert (gpu_mod._stage_need(batch)
                <= int(gpu_mod.require_lib().crawl_stage_budget()))
    res = _run(gpu_mod, monkeypatch, writer, batch)
    _check(gpu_mod, res, _oracle(corpus, batch), writer)


@pytest.mark.parametrize("which", ["stage_at", "stage_over"])
@pytest.mark.parametrize("writer", WRITERS)
def test_stage_gate_boundary(gpu_mod, monkeypatch, writer, which):
    """Staged bytes == budget still picks the staged writer; one byte
    more falls back to the plain one. Both byte-exact, under every
    writer."""
    batch = _batch(which)
    budget = int(gpu_mod.require_lib().crawl_stage_budget())
    need = gpu_mod._stage_need(batch)
    assert need == (budget if which == "stage_at" else budget + 1)
    expect = writer
    if writer == "staged" and which == "stage_over":
        expect = "plain"
    res = _run(gpu_mod, monkeypatch, writer, batch)
    _check(gpu_mod, res, _oracle(which, batch), expect)


@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("writer", WRITERS)
def test_grid_stride_reuses_wave_state(gpu_mod, monkeypatch, writer, grid):
    """grid=1: each of the 4 waves walks 30 lines, reusing its LDS
    stage / link list / line buffer across iterations."""
    batch = _batch("fuzz22")
    assert batch.n == 120
    res = _run(gpu_mod, monkeypatch, writer, batch, grid=grid)
    _check(gpu_mod, res, _oracle("fuzz22", batch), writer)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 7])
@pytest.mark.parametrize("writer", WRITERS)
def test_small_batches(gpu_mod, monkeypatch, writer, n):
    """n % 4 != 0: some waves of the last block get no line."""
    full = _batch("fuzz22")
    idx = (torch.arange(n) * 17 + 3) % full.n
    batch = B.select_rows(full, idx)
    res = _run(gpu_mod, monkeypatch, writer, batch)
    _check(gpu_mod, res, _oracle(("fuzz22", n), batch), writer)


@pytest.mark.parametrize("writer", WRITERS)
def test_median_filter_interleaves(gpu_mod, monkeypatch, writer):
    batch = _batch("fuzz33")
    cutoff = C.median_cutoff(batch)
    oracle = _oracle(("fuzz33", "median"), batch, min_post_date=cutoff)
    kept = sum(1 for l in oracle[0] if l)
    assert 0 < kept < batch.n
    res = _run(gpu_mod, monkeypatch, writer, batch, min_post_date=cutoff)
    _check(gpu_mod, res, oracle, writer)


@pytest.mark.parametrize("writer", WRITERS)
def test_filter_drops_everything(gpu_mod, monkeypatch, writer):
    batch = _batch("fuzz33")
    cutoff = C.future_cutoff(batch)
    oracle = _oracle(("fuzz33", "future"), batch, min_post_date=cutoff)
    assert all(l == b"" for l in oracle[0])
    res = _run(gpu_mod, monkeypatch, writer, batch, min_post_date=cutoff)
    _check(gpu_mod, res, oracle, writer)
    assert res.out.numel() == 0
    assert int(res.line_len.abs().sum().item()) == 0
    assert int(res.link_cnt.abs().sum().item()) == 0


@pytest.mark.parametrize("single_pass", [False, True])
def test_empty_batch(gpu_mod, monkeypatch, single_pass):
    """n = 0 launches nothing and equals the oracle's ([], [])."""
    monkeypatch.delenv("CRAWL_NO_STAGED", raising=False)
    monkeypatch.delenv("CRAWL_LDS_WRITE", raising=False)
    batch = B.pack([], [], [])
    oracle = encode_batch(batch, now=C.NOW)
    assert oracle == ([], [])
    res = gpu_mod.parse_encode(batch.to("cuda:0"), now=C.NOW,
                               single_pass=single_pass,
                               _poison=POISON, _guard=GUARD)
    torch.cuda.synchronize()
    _check(gpu_mod, res, oracle, "")
    assert res.out.numel() == 0
    assert tuple(res.link_name.shape) == (0, gpu_mod.MAX_LINKS, 32)
    assert res.link_name.dtype == torch.uint8
    for t in (res.link_len, res.link_src):
        assert tuple(t.shape) == (0, gpu_mod.MAX_LINKS)
        assert t.dtype == torch.uint8
    assert tuple(res.link_hash.shape) == (0, gpu_mod.MAX_LINKS)
    assert res.link_hash.dtype == torch.int64
    assert tuple(res.link_cnt.shape) == (0,)
    assert res.link_cnt.dtype == torch.int32
    # and with the seams off (today's allocation path)
    res = gpu_mod.parse_encode(batch.to("cuda:0"), now=C.NOW,
                               single_pass=single_pass)
    assert res.out.numel() == 0 and res.raw is None
    assert gpu_mod.links_to_python(res) == []
