"""Oracle-only checks that the shared corpora (tests/_corpora.py) really
have the properties the GPU writer/seen-set tests rely on. Runs on a
machine without a GPU or the HIP library."""
import json

import _corpora as C
from crawler_amd.ops import batch as B
from crawler_amd.ops import gpu
from crawler_amd.ops.golden_batch import encode_batch


def _escaped_growth(text):
    """Extra bytes the Go-JSON escaping adds to ``text``."""
    return len(json.dumps(text, ensure_ascii=False).encode("utf-8")) - 2 \
        - len(text.encode("utf-8"))


def test_lds_ladder_straddles_the_line_buffer():
    batch = C.lds_ladder()
    lines, _ = encode_batch(batch, now=C.NOW)
    lens = [len(l) for l in lines]
    assert {3070, 3071, 3072, 3073, 3074} <= set(lens)
    assert C.LDS_LINE_BYTES == 3072
    # the escape rows fit the buffer raw and overflow it once escaped
    rows = C.lds_ladder_escape_rows()
    assert len(rows) == 2
    for i in rows:
        text = B.unpack_message(batch, i).text.text
        growth = len(lines[i]) - len(
            encode_batch(_unescaped_twin(batch, i), now=C.NOW)[0][0])
        assert growth > 0
        assert len(lines[i]) > C.LDS_LINE_BYTES
        assert len(lines[i]) - growth <= C.LDS_LINE_BYTES
        for ch in ('"', "<", "\n", "\u2028"):
            assert text.count(ch) >= 40
    # lines that go through the LDS copy start at every residue mod 4
    off, residues = 0, set()
    for n in lens:
        if n <= C.LDS_LINE_BYTES:
            residues.add(off % 4)
        off += n
    assert residues == {0, 1, 2, 3}
    # every other row is clean ASCII: one output byte per text byte
    for i in range(batch.n):
        if i not in rows:
            assert B.unpack_message(batch, i).text.text.isalnum()


def _unescaped_twin(batch, i):
    """Row i alone, with its text replaced by clean ASCII of the same
    byte length (what the line would measure without escaping)."""
    m = B.unpack_message(batch, i)
    m.text.text = "z" * len(m.text.text.encode("utf-8"))
    return B.pack([m], [B.channel_row(batch, 0)], [0])


def test_stage_ladder_lands_on_the_gate_boundary():
    budget, fixed = 3968, 812
    assert gpu._STAGE_FIXED == fixed
    at, over = C.stage_ladder(budget, fixed)
    for batch, want in ((at, budget), (over, budget + 1)):
        m = batch.meta
        need = (fixed
                + max(int(m["text_len"].max()), int(m["aux_len"].max()))
                + int(m["poster_len"].max())
                + int(batch.ch_user_len.max())
                + int(batch.ch_title_len.max()))
        assert need == want
        assert gpu._stage_need(batch) == want
        assert gpu._pick_writer({}, False, need, budget) == (
            "staged" if want == budget else "plain")
        # text (row 0) and aux (row 1) both sit at the maximum
        assert int(m["text_len"][0]) == int(m["aux_len"][1]) \
            == max(int(m["text_len"].max()), int(m["aux_len"].max()))
        assert B.CONTENT_TYPES[int(m["content_type"][1])] \
            == "messageDocument"
        lines, links = encode_batch(batch, now=C.NOW)
        assert len(links[0]) == 8 and len(set(links[0])) == 8
        post = json.loads(lines[0])
        assert len(post["reactions"]) == len(B.EMOJI_TABLE) == 10
        # the aux-sourced description made it into the line
        assert json.loads(lines[1])["description"].startswith('doc "n" <&> d')
        # channel strings carry escapes
        assert _escaped_growth(B.channel_row(batch, 0).title) > 0


def test_median_filter_keeps_about_half():
    batch = C.fuzz_batch(33)
    assert batch.n == 120
    lines, links = encode_batch(batch, now=C.NOW,
                                min_post_date=C.median_cutoff(batch))
    kept = [bool(l) for l in lines]
    assert 0.25 * batch.n <= sum(kept) <= 0.75 * batch.n
    # kept and filtered rows interleave rather than forming two blocks
    flips = sum(1 for a, b in zip(kept, kept[1:]) if a != b)
    assert flips >= 20
    lines, links = encode_batch(batch, now=C.NOW,
                                min_post_date=C.future_cutoff(batch))
    assert all(l == b"" for l in lines) and all(r == [] for r in links)


def test_fuzz_batches_fit_the_staged_writer():
    for seed in (11, 22, 33):
        assert gpu._stage_need(C.fuzz_batch(seed)) <= 3968
    for batch in (C.edge_batch()[1], C.swar_batch()[1], C.lds_ladder()):
        assert gpu._stage_need(batch) <= 3968


def test_seenset_hash_sets():
    last, first = C.wrap_chain_hashes()
    assert len(last) == 40 and len(first) == 8
    assert all(h & 63 == 63 for h in last)
    assert all(h & 63 == 0 for h in first)
    assert len(set(last + first)) == 48
    assert not {0, 1} & set(last + first)
    assert any(h >> 63 for h in last + first)
    dups = C.dup_hashes()
    assert len(set(dups)) == 16 and not {0, 1} & set(dups)
    one, two = C.bloom_hashes()
    assert 0 in one and any(h >> 63 for h in one)
    assert len(set(one)) == len(one) and len(set(two)) == len(two)
    assert set(two) - set(one)
    for home, count, log2, salt in ((5, 20, 10, 7), (9, 5, 8, 50),
                                    (3, 12, 10, 90)):
        hs = C.home_slot_hashes(home, count, log2, salt=salt)
        assert len(set(hs)) == count
        assert all(h & ((1 << log2) - 1) == home for h in hs)
        assert all(1 < h < (1 << 64) for h in hs)


def test_pick_writer_truth_table():
    budget = 3968
    for lds in (None, "1"):
        for no_staged in (None, "1", "0"):
            for single_pass in (False, True):
                for need in (None, 812, budget, budget + 1):
                    env = {}
                    if lds is not None:
                        env["CRAWL_LDS_WRITE"] = lds
                    if no_staged is not None:
                        env["CRAWL_NO_STAGED"] = no_staged
                    if single_pass:
                        want = "scratch"
                    elif lds:
                        want = "lds"
                    elif no_staged == "1":
                        want = "plain"
                    elif need is not None and need <= budget:
                        want = "staged"
                    else:
                        want = "plain"
                    got = gpu._pick_writer(env, single_pass, need, budget)
                    assert got == want, (env, single_pass, need)
    # spelled out: the default path and each override
    assert gpu._pick_writer({}, False, 900, budget) == "staged"
    assert gpu._pick_writer({}, False, budget, budget) == "staged"
    assert gpu._pick_writer({}, False, budget + 1, budget) == "plain"
    assert gpu._pick_writer({}, False, None, budget) == "plain"
    assert gpu._pick_writer({"CRAWL_NO_STAGED": "1"}, False, 900,
                            budget) == "plain"
    assert gpu._pick_writer({"CRAWL_LDS_WRITE": "1"}, False, 900,
                            budget) == "lds"
    assert gpu._pick_writer({"CRAWL_LDS_WRITE": "1",
                             "CRAWL_NO_STAGED": "1"}, False, 900,
                            budget) == "lds"
    assert gpu._pick_writer({"CRAWL_LDS_WRITE": "1"}, True, 900,
                            budget) == "scratch"
    # an empty CRAWL_LDS_WRITE is "unset" (truthiness, as before)
    assert gpu._pick_writer({"CRAWL_LDS_WRITE": ""}, False, 900,
                            budget) == "staged"


def test_stride_bound_handles_row_subsets():
    """The single-pass scratch stride must bound every line of a
    select_rows() batch, whose comment table is the parent's (shared
    pools), not the selected rows' segments laid end to end."""
    import torch

    full = C.fuzz_batch(22)
    lines, _ = encode_batch(full, now=C.NOW)
    assert gpu._stride_bound(full) >= max(len(l) for l in lines)
    with_comments = [i for i in range(full.n)
                     if int(full.meta["com_cnt"][i])]
    assert len(with_comments) >= 3
    for idx in ([with_comments[2]], with_comments[::-1][:5],
                [(k * 17 + 3) % full.n for k in range(7)]):
        sub = B.select_rows(full, torch.tensor(idx))
        sub_lines, _ = encode_batch(sub, now=C.NOW)
        assert sub_lines == [lines[i] for i in idx]
        bound = gpu._stride_bound(sub)
        assert bound >= max(len(l) for l in sub_lines)
        # per-row bounds are the parent's: the subset's max is among them
        assert bound <= gpu._stride_bound(full)


def test_empty_batch_oracle():
    assert encode_batch(B.pack([], [], []), now=C.NOW) == ([], [])


# ------------------------------------------------------- YouTube corpora

def _yt_rows(batch):
    from crawler_amd.youtube.batch import unpack_video

    return [unpack_video(batch, i) for i in range(batch.n)]


def _yt_lines(batch):
    from crawler_amd.youtube.batch import encode_yt_batch

    return [json.loads(l) for l in encode_yt_batch(batch, now=C.NOW)]


def test_yt_corpora_are_utf8_without_the_poison_byte():
    corpora = C.yt_corpora()
    assert len(corpora) >= 15
    for name, batch in corpora.items():
        assert 1 <= batch.n <= 40, name
        pool = bytes(batch.pool.numpy())
        pool.decode("utf-8")                       # strict
        assert C.YT_POISON not in pool, name
        label = batch.crawl_label.encode("utf-8")
        assert C.YT_POISON not in label, name
        _yt_rows(batch)                            # every field decodes
    for now in (C.NOW, C.NOW.replace(microsecond=0)):
        from crawler_amd.models.post import format_go_time

        assert C.YT_POISON not in format_go_time(now).encode()


def _year(secs):
    return C._yt_time(secs).year


def test_yt_corpora_stay_inside_the_declared_domains():
    lo, hi = C.YT_DATES[0], C.YT_DATES[-1]
    assert _year(lo) == 1 and _year(hi) == 9999
    for name, batch in C.yt_corpora().items():
        v = batch.views.numpy()
        assert v.min() >= 0 and v.max() <= C.YT_MAX_VIEWS, name
        assert C.YT_MAX_VIEWS == 2 ** 53
        for t in (batch.published, batch.ch_published):
            assert int(t.min()) >= lo and int(t.max()) <= hi, name
        for t in (batch.likes, batch.comments, batch.ch_videos,
                  batch.ch_subs, batch.ch_views):
            assert int(t.min()) >= 0, name
        assert int(batch.duration_s.min()) >= -1, name
        assert int(batch.channel_idx.min()) >= 0
        assert int(batch.channel_idx.max()) < batch.n_channels


def test_yt_url_edges_provoke_what_they_claim():
    batch = C.yt_url_edges()
    posts = _yt_lines(batch)
    by_desc = {p["description"]: p["outlinks"] for p in posts}
    # bare schemes: no URL at all
    for d in ("see http:// x", "http://<b", "bare at end http://",
              "bare at end https://"):
        assert by_desc[d] == [], d
    assert by_desc["HTTP://a Http://b hTTps://c"] == []
    assert by_desc["hthttp://a"] == ["http://a"]
    assert by_desc["httphttp://a"] == ["http://a"]
    assert by_desc["http://a<http://b"] == ["http://a", "http://b"]
    assert by_desc["https://a.b/c).,"] == ["https://a.b/c"]
    assert by_desc["http://."] == ["http://"]
    # more than 8 distinct URLs survive, in first-appearance order
    counts = sorted(len(p["outlinks"]) for p in posts)
    assert {9, 10, 40} <= set(counts)
    many = [p for p in posts if len(p["outlinks"]) == 40][0]
    assert many["outlinks"] == many["description"].split(" ")
    twelve = [p for p in posts
              if p["description"].startswith("https://d.example/0 ")][0]
    assert len(twelve["description"].split(" ")) == 12
    assert twelve["outlinks"] == ["https://d.example/%d" % j
                                  for j in range(8)]
    # the continuing bytes stay inside the URL; the real stops end it
    for ch in ("\x01", "\x0b", "\x7f", "\u00a0", "\u2028"):
        assert by_desc["http://a%sb c" % ch] == ["http://a%sb" % ch]
    stops = [p for p in posts if p["description"].startswith("http://s0")][0]
    assert stops["outlinks"] == ["http://s%d" % j for j in range(8)]
    trims = [p for p in posts
             if p["description"].startswith("x https://t0.")][0]
    assert trims["outlinks"] == ["https://t%d.example/c" % j
                                 for j in range(10)]
    # a URL that needs escaping
    assert by_desc[[d for d in by_desc if d.startswith("https://e.sc")][0]] \
        == ["https://e.sc/?a=1&b=2\\c&d"]
    # the baits: row i's description is followed by row i+1's id in the
    # pool, and that id would extend or complete a URL
    pool = bytes(batch.pool.numpy())
    for text, bait, want in (
            ("bare at end http://", "x.example/y", []),
            ("end http://tail.example/p", "ath/http://",
             ["http://tail.example/p"]),
            ("see htt", "p://abc.de/", [])):
        i = [k for k, p in enumerate(posts) if p["description"] == text][0]
        end = int(batch.desc_off[i]) + int(batch.desc_len[i])
        assert pool[end:end + 11] == bait.encode()
        assert int(batch.vid_off[i + 1]) == end
        assert posts[i]["outlinks"] == want
        # ... and reading on WOULD change the answer
        from crawler_amd.youtube.convert import extract_urls

        assert extract_urls(text + bait + " ") != want


def test_yt_sanitize_edges_hit_the_cap():
    from crawler_amd.youtube.convert import sanitize_filename

    rows = _yt_rows(C.yt_sanitize_edges())
    names = {v.title: sanitize_filename(v.title) for v, _ in rows}
    assert names[""] == "" and names["!!!"] == "_"
    assert names["s" * 79 + "!!y"] == "s" * 79 + "_"
    assert names["s" * 80 + "more"] == "s" * 80
    assert names["a!" * 60] == "a_" * 40
    assert names["!" * 200 + "x"] == "_x"
    assert names["\u00e9" * 3] == "_"
    assert names["a\U0001F680b"] == "a_b"
    assert names["keep.dots-and_under"] == "keep.dots-and_under"
    lens = [len(n) for n in names.values()]
    assert lens.count(80) >= 4 and max(lens) == 80
    posts = _yt_lines(C.yt_sanitize_edges())
    assert any(p["media_data"]["document_name"]
               == p["post_uid"] + "-" + "a_" * 40 + ".mp4" for p in posts)


def test_yt_esc_ladder_covers_lengths_and_block_straddles():
    batches = C.yt_esc_ladder()
    titles = [v.title.encode() for b in batches for v, _ in _yt_rows(b)]
    assert {len(t) for t in titles} >= set(C.YT_ESC_LENGTHS)
    # a U+2028 over byte 256 of a field, at every split
    u = "\u2028".encode()
    starts = {t.index(u) for t in titles if u in t}
    assert {253, 254, 255, 256, 509, 510, 511, 512} <= starts
    for sp in (b'"', b"\\", b"\n", b"<", b"&", b"\x01"):
        for p in (255, 256):
            assert any(len(t) == 513 and t[p:p + 1] == sp
                       and t.count(sp) == 1 for t in titles)
        # first and last byte of some string
        assert any(t[:1] == sp for t in titles)
        assert any(t[-1:] == sp for t in titles)
    dash = "\u2014".encode()
    assert {t.index(dash) for t in titles if dash in t} >= {253, 254,
                                                            255, 256}
    # the same strings reach the channel fields, and every label is used
    ch_fields = set()
    for b in batches:
        for _, ch in _yt_rows(b):
            ch_fields |= {ch.title, ch.description, ch.country}
    assert any(len(s.encode()) == 1030 for s in ch_fields)
    assert any("\u2028" in s for s in ch_fields)
    assert [b.crawl_label for b in batches[-3:]] == C.YT_LABELS
    assert len(C.YT_LABELS[2].encode()) == 300
    line = _yt_lines(batches[-2])[0]
    assert line["crawl_label"] == C.YT_LABELS[1]


def test_yt_number_edges_cover_the_digit_ladder():
    batch = C.yt_number_edges()
    views = set(batch.views.tolist())
    want = {0, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 53 - 1, 2 ** 53}
    for k in range(1, 16):
        want |= {10 ** k - 1, 10 ** k}
    assert want <= views
    for t in (batch.ch_subs, batch.ch_views):
        assert (want - {2 ** 53 - 1, 2 ** 53}) | {2 ** 63 - 1} \
            <= set(t.tolist())
    i32 = 2 ** 31 - 1
    for t in (batch.likes, batch.comments, batch.ch_videos):
        assert {0, i32} <= set(t.tolist())
    assert set(batch.duration_s.tolist()) == {-1, 0, 1, i32}
    assert set(batch.lang.tolist()) == {0, 1}
    assert set(batch.published.tolist()) == set(C.YT_DATES)
    assert set(batch.ch_published.tolist()) == set(C.YT_DATES)
    posts = _yt_lines(batch)
    assert max(p["engagement"] for p in posts) > 2 ** 32   # past int32
    assert any(p["like_count"] == i32 and p["comment_count"] == i32
               for p in posts)
    stamps = {p["published_at"] for p in posts}
    assert {"0001-01-01T00:00:00Z", "1969-12-31T23:59:59Z",
            "1970-01-01T00:00:00Z", "2000-02-29T00:00:00Z",
            "2100-03-01T00:00:00Z", "1972-02-29T00:00:00Z",
            "9999-12-31T23:59:59Z"} == stamps
    # the float field prints the exact integer over the whole domain
    for p in posts:
        assert p["performance_scores"]["views"] == p["view_count"]
    raw = C.encode_yt_lines(batch)
    assert any(b'"views":9007199254740992}' in l for l in raw)
    assert {None, 0, 1, i32} == {p["video_length"] for p in posts}


def test_yt_shape_batches_share_and_reorder_channels():
    shapes = C.yt_shape_batches()
    assert sorted(shapes) == [1, 2, 3, 5, 7, 9]
    from crawler_amd.youtube.batch import encode_yt_batch

    full = shapes[9]
    lens = [len(l) for l in encode_yt_batch(full, now=C.NOW)]
    assert max(lens) > 1.8 * min(lens)
    idx = full.channel_idx.tolist()
    assert len(set(idx)) < len(idx)                   # shared channels
    first_seen = list(dict.fromkeys(idx))
    assert first_seen != sorted(first_seen)           # table order differs
    for n, b in shapes.items():
        assert b.n == n and b.n_channels == 4
    # capture_time's length follows now's fraction
    assert len({len(encode_yt_batch(
        full, now=C.NOW.replace(microsecond=m))[0])
        for m in (0, 890000, 5)}) == 3
