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
