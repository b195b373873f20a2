"""Edge matrices for the three aux kernels, each against a plain oracle:

- ``channel_stats`` (csrc/aggregate.hip) vs numpy int64 sums: P around
  the wave and block sizes, values at the int32 extremes, ``line_len``,
  no channels, and output guards;
- ``reservoir_sample`` (csrc/sample.hip) vs ``reservoir_sample_oracle``
  (whose uniformity test_aux_corpora_preconditions checks on the CPU):
  k from 0 to past P, seeds over the 64-bit range, one block striding
  over the channels, and output guards;
- ``html_classify`` (csrc/htmlclass.hip) vs ``parse_channel_html`` on the
  ``html_*`` corpora of tests/_corpora.py: the regex semantics, the
  64-lane search window's edges, the 64 KiB cap, back-to-back packing,
  one block striding over the documents, and output guards.
"""
import datetime as dt
import functools

import numpy as np
import pytest
import torch

import _corpora as C
from crawler_amd.feed import FeedConfig, SyntheticFeed
from crawler_amd.ops import batch as B
from crawler_amd.ops import gpu
from crawler_amd.ops.golden_batch import encode_batch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


@functools.lru_cache(maxsize=None)
def _feed():
    return SyntheticFeed(FeedConfig(seed=9, universe=1000))


@functools.lru_cache(maxsize=None)
def _cpu_batch(K, P):
    return _feed().build_batch(np.arange(K, dtype=np.int64),
                               posts_per_channel=P)


def _dev_batch(K, P):
    """A fresh device copy: the tests overwrite its meta tensors."""
    return _cpu_batch(K, P).to(DEV)


# ------------------------------------------------------------ channel_stats

def _stat_fields(K, P):
    """{name: (views, forwards, replies)} int32 arrays of K*P slots."""
    n = K * P
    i = np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(1000 * K + P)
    full = lambda v: np.full(n, v, dtype=np.int64)
    alt = np.where(i % 2 == 0, I32_MAX, I32_MIN)
    rnd = lambda: rng.integers(I32_MIN, I32_MAX, n, endpoint=True)
    fields = {
        "max": (full(I32_MAX),) * 3,
        "min": (full(I32_MIN),) * 3,
        "alternating": (alt, np.where(i % 3 == 0, I32_MIN, I32_MAX),
                        np.where(i % 3 == 0, -7, 5)),
        "distinct": (i % 1000, 7 * i + 1, -(i % 13)),
        "random": (rnd(), rnd(), rnd()),
    }
    return {k: tuple(a.astype(np.int32) for a in v)
            for k, v in fields.items()}


def _stats_oracle(K, P, v, f, r, line_len=None):
    s = lambda a: a.astype(np.int64).reshape(K, P).sum(axis=1)
    posts = (np.full(K, P, dtype=np.int64) if line_len is None
             else (line_len.reshape(K, P) > 0).sum(axis=1))
    return {"views": s(v), "forwards": s(f), "replies": s(r),
            "posts": posts,
            "totals": np.array([s(v).sum(), s(f).sum(), s(r).sum(),
                                posts.sum()], dtype=np.int64)}


def _assert_stats(out, want):
    assert sorted(out) == sorted(want)
    for name, w in want.items():
        got = out[name]
        assert got.dtype == (torch.int32 if name == "posts"
                             else torch.int64), name
        assert got.cpu().numpy().tolist() == w.tolist(), name


def _set_fields(batch, v, f, r):
    for name, a in (("views", v), ("forwards", f), ("reply_count", r)):
        batch.meta[name] = torch.from_numpy(a).to(DEV)


@pytest.mark.parametrize("K", [1, 3, 17])
@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_channel_stats_matrix(K, P):
    batch = _dev_batch(K, P)
    for name, (v, f, r) in _stat_fields(K, P).items():
        _set_fields(batch, v, f, r)
        out = gpu.channel_stats(batch)
        torch.cuda.synchronize()
        _assert_stats(out, _stats_oracle(K, P, v, f, r))


def test_channel_stats_sums_pass_int32_and_uint32():
    K, P = 3, 1000
    v, f, r = _stat_fields(K, P)["max"]
    want = _stats_oracle(K, P, v, f, r)
    assert want["views"][0] > 2 ** 32 and want["totals"][0] > 2 ** 33
    v, f, r = _stat_fields(K, P)["min"]
    want = _stats_oracle(K, P, v, f, r)
    assert want["views"][0] < -2 ** 32 and want["totals"][0] < -2 ** 33
    # the three fields of "distinct" and "alternating" differ per channel
    for name in ("distinct", "alternating"):
        w = _stats_oracle(K, P, *_stat_fields(K, P)[name])
        assert len({tuple(w[k].tolist())
                    for k in ("views", "forwards", "replies")}) == 3


@pytest.mark.parametrize("K,P", [(1, 1), (3, 65), (17, 257)])
def test_channel_stats_line_len(K, P):
    batch = _dev_batch(K, P)
    v, f, r = _stat_fields(K, P)["distinct"]
    _set_fields(batch, v, f, r)
    i = np.arange(K * P)
    for ll in (np.select([i % 5 == 0, i % 5 == 1, i % 5 == 2],
                         [0, -3, I32_MAX], default=1 + i % 900),
               np.zeros(K * P), np.full(K * P, -1), np.full(K * P, 17)):
        ll = ll.astype(np.int32)
        out = gpu.channel_stats(batch, torch.from_numpy(ll).to(DEV))
        torch.cuda.synchronize()
        _assert_stats(out, _stats_oracle(K, P, v, f, r, ll))


def test_channel_stats_counts_the_lines_a_date_filter_keeps():
    K, P = 3, 65
    now = dt.datetime(2026, 1, 1, tzinfo=dt.timezone.utc)
    cpu_b = _cpu_batch(K, P)
    dates = np.sort(cpu_b.meta["date"].numpy())
    cutoff = dt.datetime.fromtimestamp(int(dates[len(dates) // 3]),
                                       dt.timezone.utc)
    batch = _dev_batch(K, P)
    res = gpu.parse_encode(batch, now=now, min_post_date=cutoff)
    out = gpu.channel_stats(batch, res.line_len)
    torch.cuda.synchronize()
    lines, _ = encode_batch(cpu_b, now=now, min_post_date=cutoff)
    kept = np.array([len(l) > 0 for l in lines]).reshape(K, P)
    assert 0 < kept.sum() < K * P
    assert res.line_len.cpu().numpy().tolist() == [len(l) for l in lines]
    m = cpu_b.meta
    want = _stats_oracle(K, P, m["views"].numpy(), m["forwards"].numpy(),
                         m["reply_count"].numpy(),
                         np.array([len(l) for l in lines]))
    assert want["posts"].tolist() == kept.sum(axis=1).tolist()
    _assert_stats(out, want)


def test_channel_stats_refuses_a_line_len_it_cannot_read(monkeypatch):
    K, P = 3, 5
    batch = _dev_batch(K, P)
    C.forbid_launches(monkeypatch)
    n = K * P
    for bad in (torch.ones(n, dtype=torch.int64, device=DEV),
                torch.ones(n, dtype=torch.int16, device=DEV),
                torch.ones(n, dtype=torch.float32, device=DEV),
                torch.ones(n - 1, dtype=torch.int32, device=DEV),
                torch.ones(n + 1, dtype=torch.int32, device=DEV),
                torch.ones(0, dtype=torch.int32, device=DEV),
                torch.ones(n, dtype=torch.int32)):
        with pytest.raises(ValueError):
            gpu.channel_stats(batch, bad)


def test_channel_stats_without_channels(monkeypatch):
    batch = _feed().build_batch(np.zeros(0, dtype=np.int64),
                                posts_per_channel=5).to(DEV)
    C.forbid_launches(monkeypatch)
    for line_len in (None, torch.zeros(0, dtype=torch.int32, device=DEV)):
        out = gpu.channel_stats(batch, line_len)
        _assert_stats(out, _stats_oracle(0, 5, *(np.zeros(0, np.int32),) * 3))
        assert out["totals"].tolist() == [0, 0, 0, 0]


_POISON64 = -0x5A5A5A5A5A5A5A5B
_POISON32 = -0x5A5A5A5B


def _guarded(n, dtype, fill, pad=8):
    """(buffer, view): ``n`` slots with ``pad`` poisoned ones each side;
    the view is poisoned too."""
    raw = torch.full((n + 2 * pad,), fill, dtype=dtype, device=DEV)
    return raw, raw[pad:pad + n]


def _assert_guards(raw, n, fill, pad=8):
    a = raw.cpu()
    assert (a[:pad] == fill).all() and (a[pad + n:] == fill).all()


@pytest.mark.parametrize("K,P", [(1, 1), (3, 65), (17, 257)])
def test_channel_stats_writes_only_its_outputs(K, P):
    """The entry point itself, with outputs that are slices of poisoned
    buffers. The kernel ADDS into ``totals`` (one atomic per channel):
    the caller zeroes it, as ``gpu.channel_stats`` does; the per-channel
    outputs are plain stores and need no initial value."""
    v, f, r = _stat_fields(K, P)["random"]
    ll = (np.arange(K * P) % 3).astype(np.int32)
    want = _stats_oracle(K, P, v, f, r, ll)
    t = lambda a: torch.from_numpy(a).to(DEV)
    bufs = {name: _guarded(K, torch.int64, _POISON64)
            for name in ("views", "forwards", "replies")}
    bufs["posts"] = _guarded(K, torch.int32, _POISON32)
    bufs["totals"] = _guarded(4, torch.int64, _POISON64)
    bufs["totals"][1].zero_()
    gpu._call("crawl_channel_stats", t(v), t(f), t(r), t(ll), P, K,
              bufs["views"][1], bufs["forwards"][1], bufs["replies"][1],
              bufs["posts"][1], bufs["totals"][1])
    torch.cuda.synchronize()
    _assert_stats({k: view for k, (_, view) in bufs.items()}, want)
    for name, (raw, view) in bufs.items():
        _assert_guards(raw, view.numel(),
                       _POISON32 if name == "posts" else _POISON64)
    # totals accumulate: a second call doubles them and nothing else
    gpu._call("crawl_channel_stats", t(v), t(f), t(r), t(ll), P, K,
              bufs["views"][1], bufs["forwards"][1], bufs["replies"][1],
              bufs["posts"][1], bufs["totals"][1])
    torch.cuda.synchronize()
    want["totals"] = 2 * want["totals"]
    _assert_stats({k: view for k, (_, view) in bufs.items()}, want)


# --------------------------------------------------------- reservoir_sample

_SEEDS = [0, 123, -1, 2 ** 63 - 1, 2 ** 63]


def _assert_sample(got, K, P, k, seed):
    assert got.dtype == torch.int32 and got.shape == (K, min(k, P))
    rows = got.cpu().numpy().tolist()
    assert rows == gpu.reservoir_sample_oracle(P, K, k, seed), (K, P, k,
                                                                seed)
    for c in range(K):
        assert len(set(rows[c])) == min(k, P)
        assert all(c * P <= r < (c + 1) * P for r in rows[c])


@pytest.mark.parametrize("K", [1, 4, 5, 9])
@pytest.mark.parametrize("P", [1, 2, 64, 257])
def test_reservoir_sample_matrix(K, P):
    batch = _dev_batch(K, P)
    for k in sorted({0, 1, P - 1, P}):
        for seed in _SEEDS:
            got = gpu.reservoir_sample(batch, k, seed=seed)
            torch.cuda.synchronize()
            _assert_sample(got, K, P, k, seed)


@pytest.mark.parametrize("P", [1, 2, 64, 257])
def test_reservoir_sample_one_block_strides_over_the_channels(P,
                                                              monkeypatch):
    K = 9  # three trips of a 4-wave block
    batch = _dev_batch(K, P)
    plain = {k: gpu.reservoir_sample(batch, k, seed=123)
             for k in sorted({1, P - 1, P} - {0})}
    seen = C.force_grid_one(monkeypatch, ("crawl_reservoir_sample",))
    for k, want in plain.items():
        got = gpu.reservoir_sample(batch, k, seed=123)
        torch.cuda.synchronize()
        _assert_sample(got, K, P, k, 123)
        assert torch.equal(got, want)
    assert len(seen) == len(plain)


@pytest.mark.parametrize("P,k", [(3, 5), (1, 2), (3, 3), (3, 2 ** 31 - 1)])
def test_reservoir_sample_keeps_a_small_channel_whole(P, k):
    """k >= P: every row of every channel, and no index leaves its
    channel (telegramutils.go:124 keeps all messages when there are no
    more than sample_size)."""
    K = 5
    batch = _dev_batch(K, P)
    for seed in _SEEDS:
        got = gpu.reservoir_sample(batch, k, seed=seed)
        torch.cuda.synchronize()
        _assert_sample(got, K, P, k, seed)
        assert got.cpu().tolist() == [list(range(c * P, (c + 1) * P))
                                      for c in range(K)]


def test_reservoir_sample_edges_without_a_launch(monkeypatch):
    C.forbid_launches(monkeypatch)
    empty = _feed().build_batch(np.zeros(0, dtype=np.int64),
                                posts_per_channel=5).to(DEV)
    assert gpu.reservoir_sample(empty, 3).shape == (0, 0)
    assert gpu.reservoir_sample(_dev_batch(4, 2), 0).shape == (4, 0)
    with pytest.raises(ValueError):
        gpu.reservoir_sample(_dev_batch(4, 2), -1)


@pytest.mark.parametrize("k", [7, 200, 500])
def test_sample_select_encode_matches_golden(k):
    """sample -> select_rows -> parse_encode, at k < P, k = P and k > P."""
    now = dt.datetime(2026, 1, 1, tzinfo=dt.timezone.utc)
    K, P = 3, 200
    batch = _dev_batch(K, P)
    idx = gpu.reservoir_sample(batch, k, seed=5)
    assert idx.shape == (K, min(k, P))
    sub_idx = idx.flatten()
    res = gpu.parse_encode(B.select_rows(batch, sub_idx), now=now)
    torch.cuda.synchronize()
    lines, _ = encode_batch(B.select_rows(_cpu_batch(K, P), sub_idx.cpu()),
                            now=now)
    assert len(lines) == K * min(k, P)
    assert bytes(res.out.cpu().numpy()) == b"".join(lines)


@pytest.mark.parametrize("K,P,k", [(1, 1, 1), (5, 64, 63), (9, 257, 1)])
def test_reservoir_sample_writes_only_its_output(K, P, k):
    raw, view = _guarded(K * k, torch.int32, _POISON32)
    gpu._call("crawl_reservoir_sample", 123, P, K, k, view,
              min(max(1, (K + 3) // 4), 8192))
    torch.cuda.synchronize()
    _assert_sample(view.view(K, k), K, P, k, 123)
    _assert_guards(raw, K * k, _POISON32)


# ------------------------------------------------------------ html_classify

_CORPUS = C.html_corpus()


def _assert_classified(docs, got):
    want = C.html_oracle(docs)
    assert len(got) == len(docs)
    bad = [(i, docs[i][:120], got[i], want[i])
           for i in range(len(docs)) if got[i] != want[i]]
    assert not bad, f"{len(bad)} of {len(docs)} differ: {bad[:8]}"


@pytest.mark.parametrize("group", sorted(_CORPUS))
def test_html_corpus_matches_the_oracle(group):
    docs = _CORPUS[group]
    _assert_classified(docs, gpu.html_classify(docs))


@pytest.mark.parametrize("k", range(len(C.HTML_TABLE_ROWS)))
def test_html_table_row(k):
    doc, want = C.HTML_TABLE_ROWS[k]
    assert gpu.html_classify([doc]) == [want]


def test_html_reversed_order_lands_in_other_waves():
    docs = [d for g in sorted(_CORPUS) if g != "fuzz"
            for d in _CORPUS[g]][::-1]
    _assert_classified(docs, gpu.html_classify(docs))


def test_html_window_edges_by_kind():
    for kind in ("title_open", "title_gt", "title_close", "meta_first",
                 "meta_next", "name", "noindex"):
        rows = [e for e in C.html_window_edges() if e[0] == kind]
        got = gpu.html_classify([d for _, _, d, _ in rows])
        assert got == [w for _, _, _, w in rows], kind


def _shape_docs(n):
    docs = [d for d, _ in C.HTML_TABLE_ROWS] + C.html_short_ranges()
    return docs[:n]


@pytest.mark.parametrize("n", [0, 1, 4, 5])
def test_html_document_counts(n):
    docs = _shape_docs(n)
    assert len(docs) == n
    _assert_classified(docs, gpu.html_classify(docs))


def test_html_nine_documents_in_one_block(monkeypatch):
    docs = _shape_docs(9)
    plain = gpu.html_classify(docs)
    seen = C.force_grid_one(monkeypatch, ("crawl_html_classify",))
    got = gpu.html_classify(docs)
    assert seen == ["crawl_html_classify"]
    assert got == plain
    _assert_classified(docs, got)
    # the whole hand-made corpus through one block as well
    docs = [d for g in ("table", "rules", "packing") for d in _CORPUS[g]]
    _assert_classified(docs, gpu.html_classify(docs))


def test_html_empty_documents_first_last_and_between():
    filler = [d for d, _ in C.HTML_TABLE_ROWS]
    for docs in ([b""] + filler, filler + [b""],
                 filler[:3] + [b"", b""] + filler[3:],
                 [b"", b"", b""], [b""] + C.html_packing_docs() + [b""]):
        _assert_classified(docs, gpu.html_classify(docs))


def _pack(docs):
    blob = b"".join(docs) or b"\0"
    pool = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(DEV)
    lens = [len(d) for d in docs]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]) if docs else []
    return (pool, torch.tensor(offs, dtype=torch.int64, device=DEV),
            torch.tensor(lens, dtype=torch.int32, device=DEV))


def test_html_classify_writes_only_its_outputs():
    docs = C.html_packing_docs() + [d for d, _ in C.HTML_TABLE_ROWS]
    n = len(docs)
    pool, doc_off, doc_len = _pack(docs)
    s_raw, status = _guarded(n, torch.int32, _POISON32)
    r_raw, reason = _guarded(n, torch.int32, _POISON32)
    gpu._call("crawl_html_classify", pool, doc_off, doc_len, n, status,
              reason, (n + 3) // 4)
    torch.cuda.synchronize()
    got = [(gpu._HTML_STATUS[s], gpu._HTML_REASON[r])
           for s, r in zip(status.cpu().tolist(), reason.cpu().tolist())]
    _assert_classified(docs, got)
    _assert_guards(s_raw, n, _POISON32)
    _assert_guards(r_raw, n, _POISON32)
