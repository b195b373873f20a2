"""Oracle-only checks behind the feed-generator and aux-kernel matrices
(test_gpu_feedgen_matrix, test_gpu_aux_matrix): the corpora of
tests/_corpora.py provoke what they claim, the reservoir oracle is
uniform, the CPU sides of the contract fixes, and vectors that pin where
``parse_channel_html`` is deliberately laxer than the reference. Runs
without a GPU or the HIP library."""
import math
import re

import numpy as np
import pytest

import _corpora as C
from crawler_amd.engine.htmlvalidator import parse_channel_html
from crawler_amd.feed import FeedConfig, SyntheticFeed
from crawler_amd.ops import gpu


# ------------------------------------------------------------- feed matrix

def _cpu_batches():
    out = {}
    for name, cfg, ids, P in C.feed_cases():
        feed = SyntheticFeed(FeedConfig(**cfg))
        out[name] = (feed, feed.build_batch(np.array(ids, dtype=np.int64),
                                            posts_per_channel=P))
    return out


def test_feed_matrix_preconditions():
    cases = C.feed_cases()
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    shapes = {(len(ids), P) for _, _, ids, P in cases}
    assert set(C.FEED_SHAPES) | {C.FEED_BIG} <= shapes
    assert set(C.FEED_FORCED) <= set(C.FEED_SHAPES)
    # N off the multiples of 4 (waves per block) and of 256
    ns = {K * P for K, P in C.FEED_SHAPES}
    assert any(n % 4 for n in ns) and all(n % 256 for n in ns)
    assert C.FEED_BIG[0] * C.FEED_BIG[1] > 8192 * 4

    batches = _cpu_batches()
    # a template is known by these per-message fields
    feed = batches[names[0]][0]
    keys = [(t.text_len, len(t.aux.encode()), int(feed._ctype[i]),
             len(t.entities), int(feed._flags[i]))
            for i, t in enumerate(feed.templates)]
    assert len(set(keys)) == len(keys)
    picked, react, last_has_comment = set(), set(), False
    with_url = without_url = 0
    for name, (_, b) in batches.items():
        m = b.meta
        picked |= set(zip(m["text_len"].tolist(), m["aux_len"].tolist(),
                          m["content_type"].tolist(), m["ent_cnt"].tolist(),
                          m["flags"].tolist()))
        react |= set(m["react_cnt"].tolist())
        if b.n and b.com_text_off.numel() and int(m["com_cnt"][-1]) > 0:
            last_has_comment = True
        with_url += int((b.entities[:, 4] > 0).sum())
        without_url += int((b.entities[:, 4] == 0).sum())
    assert picked == set(keys)
    assert 0 in react and max(react) >= 3
    assert last_has_comment
    assert with_url and without_url

    # what single cases are there for
    _, b = batches["rate-1.0-one-post"]
    assert (b.meta["com_cnt"] > 0).all()
    for mc in (1, 3, 50):
        _, b = batches["rate-0.0-max-%d" % mc]
        assert b.com_text_off.numel() == 0
        _, b = batches["rate-1.0-max-%d" % mc]
        cnt = b.meta["com_cnt"]
        assert int(cnt.min()) >= 1 and int(cnt.max()) == mc
    _, b = batches["dates-wrap"]
    d = b.meta["date"]
    assert int(d.min()) < 0 < int(d.max())
    _, b = batches["ids-duplicate"]
    assert b.chat_id[:33].tolist() == b.chat_id[33:66].tolist()
    _, b = batches["universe-1"]
    assert b"c0000000000" in bytes(b.text_pool.numpy())
    pool = bytes(batches["universe-%d" % (10 ** 10 - 1)][1].text_pool.numpy())
    assert re.search(rb"c[5-9]\d{9}", pool)
    # the forced-grid runs give a 256-thread block a second trip over the
    # comments of the larger shape
    feed = SyntheticFeed(FeedConfig(**C.FEED_FORCED_CFG))
    b = feed.build_batch(np.arange(5), posts_per_channel=257)
    assert b.com_text_off.numel() > 256 and b.n > 256


def test_feed_entity_templates_give_many_rows_per_message():
    cfg, ids, P = C.FEED_ENTITY_CASE
    feed = SyntheticFeed(FeedConfig(**cfg), C.feed_entity_templates())
    b = feed.build_batch(np.array(ids, dtype=np.int64), posts_per_channel=P)
    cnt = b.meta["ent_cnt"].tolist()
    assert set(cnt) == {0, 1, 4, 70}
    # inside one message: rows that differ, with and without a url
    i = cnt.index(4)
    rows = b.entities[int(b.meta["ent_off"][i]):][:4].tolist()
    assert len({tuple(r) for r in rows}) == 4
    assert sorted(r[4] > 0 for r in rows) == [False, False, False, True]
    i = cnt.index(70)
    rows = b.entities[int(b.meta["ent_off"][i]):][:70]
    assert len(set(rows[:, 1].tolist())) == 70
    # the standard set never has more than one row per message
    assert max(len(t.entities) for t in SyntheticFeed().templates) == 1


def test_feed_seeds_change_the_batch():
    batches = _cpu_batches()
    views = [tuple(batches["seed-%d" % s][1].meta["views"].tolist())
             for s in (0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1)]
    assert len(set(views)) == 5


def test_build_batch_without_channels_is_empty():
    feed = SyntheticFeed(FeedConfig(seed=1, universe=10))
    b = feed.build_batch(np.zeros(0, dtype=np.int64), posts_per_channel=5)
    assert b.n == 0 and b.n_channels == 0
    assert b.text_pool.numel() == 0 and b.entities.shape == (0, 5)
    assert all(t.numel() == 0 for t in b.meta.values())


@pytest.mark.parametrize("mc", [0, -1])
def test_build_batch_needs_room_for_a_comment(mc):
    feed = SyntheticFeed(FeedConfig(seed=1, universe=10, comment_rate=0.5,
                                    max_comments_per_post=mc))
    with pytest.raises(ValueError):
        feed.build_batch(np.arange(2), posts_per_channel=3)
    # no comments asked for: the maximum does not matter
    feed = SyntheticFeed(FeedConfig(seed=1, universe=10, comment_rate=0.0,
                                    max_comments_per_post=mc))
    b = feed.build_batch(np.arange(2), posts_per_channel=3)
    assert b.n == 6 and b.com_text_off.numel() == 0


# -------------------------------------------------------- reservoir oracle

@pytest.mark.parametrize("P,k", [(20, 5), (7, 3), (64, 1)])
def test_reservoir_oracle_is_uniform(P, k):
    """The kernel is only ever compared with the oracle, so the oracle's
    own distribution is checked here: over S seeds every row of a channel
    is included S*k/P times, within 5 sigma of the binomial."""
    S = 4000
    counts = np.zeros((2, P), dtype=np.int64)
    first = np.zeros(P, dtype=np.int64)
    for seed in range(S):
        two = gpu.reservoir_sample_oracle(P, 2, k, seed)
        for c in range(2):
            assert len(set(two[c])) == k
            for r in two[c]:
                assert c * P <= r < (c + 1) * P
                counts[c, r - c * P] += 1
        # channel 0 does not depend on how many channels follow
        one = gpu.reservoir_sample_oracle(P, 1, k, seed)
        assert one == two[:1]
        for r in one[0]:
            first[r] += 1
    mean = S * k / P
    sigma = math.sqrt(S * (k / P) * (1 - k / P))
    worst = np.abs(counts - mean).max() / sigma
    print(f"P={P} k={k}: {counts.min()}..{counts.max()} around {mean:.0f}, "
          f"{worst:.2f} sigma")
    assert worst <= 5.0
    assert (first == counts[0]).all()


def test_reservoir_oracle_keeps_small_channels_whole():
    assert gpu.reservoir_sample_oracle(3, 2, 5) == [[0, 1, 2], [3, 4, 5]]
    assert gpu.reservoir_sample_oracle(1, 3, 2, seed=9) == [[0], [1], [2]]
    assert gpu.reservoir_sample_oracle(3, 2, 3) == [[0, 1, 2], [3, 4, 5]]
    assert gpu.reservoir_sample_oracle(4, 2, 0) == [[], []]


# ------------------------------------------------------------ HTML corpora

def test_html_table_rows_give_the_listed_answers():
    assert len(C.HTML_TABLE_ROWS) == 8
    for doc, want in C.HTML_TABLE_ROWS:
        assert C.html_oracle([doc]) == [want], doc


def test_html_corpus_covers_every_answer():
    corpus = C.html_corpus()
    assert sorted(corpus) == ["cap", "edges", "fuzz", "packing", "rules",
                              "short", "table"]
    answers = set()
    for docs in corpus.values():
        answers |= set(C.html_oracle(docs))
    assert answers == {C.HTML_VALID, C.HTML_NOT_CHANNEL, C.HTML_NOT_FOUND,
                       C.HTML_UNRECOGNIZED}
    # every rule decides some title, at the start, the middle and the end
    rules = C.html_oracle(C.html_rule_docs())
    assert {rules.count(a) >= 10 for a in answers} == {True}
    for doc, want in C.html_cap_docs():
        assert C.html_oracle([doc]) == [want]
    lens = sorted(len(d) for d, _ in C.html_cap_docs())
    assert C.HTML_CAP in lens and C.HTML_CAP + 1 in lens and 70_000 in lens


def test_html_window_edges_sit_where_they_claim():
    edges = C.html_window_edges()
    assert {o for _, o, _, _ in edges} == set(C.HTML_EDGE_OFFSETS)
    assert set(range(58, 71)) | set(range(122, 135)) \
        == set(C.HTML_EDGE_OFFSETS)
    kinds = set()
    for kind, off, doc, want in edges:
        kinds.add(kind)
        low = doc.lower()
        if kind == "title_open":
            start, at = 0, low.find(b"<title")
        elif kind == "title_gt":
            start = low.find(b"<title") + 6
            at = low.find(b">", start)
        elif kind == "title_close":
            start = low.find(b">", low.find(b"<title")) + 1
            at = low.find(b"</title>", start)
        elif kind == "meta_first":
            start, at = 0, low.find(b"<meta")
        elif kind == "meta_next":
            start = low.find(b"<meta") + 5
            at = low.find(b"<meta", start)
        elif kind == "name":
            start = low.find(b"<meta") + 6
            at = low.find(b'name="robots"', start)
        else:
            assert kind == "noindex"
            start = low.find(b'name="robots"') + 14
            at = low.find(b"noindex", start)
        assert at - start == off, (kind, off)
        assert C.html_oracle([doc]) == [want], (kind, off)
        # the pattern occurs once: missing it there changes the answer
        pat = {"title_open": b"<title", "title_gt": b">",
               "title_close": b"</title>", "meta_first": b"<meta",
               "meta_next": b"<meta", "name": b'name="robots"',
               "noindex": b"noindex"}[kind]
        assert low.count(pat, at) == (2 if kind == "title_gt" else 1)
        if kind == "meta_next":
            assert low.count(b"<meta") == 2
    assert len(kinds) == 7


def test_html_packing_docs_change_when_read_past_their_end():
    docs = C.html_packing_docs()
    assert len(docs) == 2 * (8 + 7)
    got = C.html_oracle(docs)
    for j in range(0, len(docs), 2):
        joined = C.html_oracle([docs[j] + docs[j + 1]])[0]
        assert got[j] in (C.HTML_UNRECOGNIZED, C.HTML_NOT_CHANNEL)
        assert joined in (C.HTML_VALID, C.HTML_NOT_FOUND)
        assert got[j] != joined
    short = C.html_oracle(C.html_short_ranges())
    assert {C.HTML_UNRECOGNIZED, C.HTML_NOT_CHANNEL,
            C.HTML_NOT_FOUND} <= set(short)


# where the oracle is deliberately laxer than (or differs from) the
# reference's ParseChannelHTML; the expected values follow from the
# oracle's rules (docs/TESTING.md, "t.me HTML contract decisions")
_CONTACT = b"<title>Telegram: Contact @a</title>"
_ORACLE_VECTORS = [
    # any <title ...> tag, in any case (the reference: exactly <title>)
    (b'<title lang="en">Telegram: View @a</title>', C.HTML_VALID),
    (b"<TITLE>Telegram: View @a</TITLE>", C.HTML_VALID),
    # a bare "View @" / "Contact @" prefix counts
    (b"<title>View @a</title>", C.HTML_VALID),
    (b"<title>Contact @a</title>", C.HTML_NOT_CHANNEL),
    # ... only as a prefix
    (b"<title>Please View @a</title>", C.HTML_UNRECOGNIZED),
    # "Telegram Messenger" anywhere in the title (the reference: the
    # whole title)
    (b"<title>Telegram Messenger - a new era</title>", C.HTML_NOT_FOUND),
    # either quote around robots (the reference: double quotes)
    (_CONTACT + b"<meta name='robots' content='noindex'>",
     C.HTML_NOT_FOUND),
    # every robots meta is tried (the reference: the first name="robots")
    (_CONTACT + b'<meta name="robots" content="all">'
     b'<meta name="robots" content="noindex">', C.HTML_NOT_FOUND),
    # noindex must follow the name attribute (the reference: anywhere in
    # the enclosing tag)
    (_CONTACT + b'<meta content="noindex" name="robots">',
     C.HTML_NOT_CHANNEL),
    # the tag must be a <meta (the reference: any enclosing <...>)
    (_CONTACT + b'<link name="robots" content="noindex">',
     C.HTML_NOT_CHANNEL),
    # an unterminated tag still counts (the reference: needs the '>')
    (_CONTACT + b'<meta name="robots" content="noindex"', C.HTML_NOT_FOUND),
]


@pytest.mark.parametrize("k", range(len(_ORACLE_VECTORS)))
def test_html_oracle_contract_vectors(k):
    doc, want = _ORACLE_VECTORS[k]
    r = parse_channel_html(doc)
    assert (r.status, r.reason) == want
