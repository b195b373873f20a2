"""Shared test corpora for the HIP parse+encode writers and the seen-set.

Everything here is CPU-only: builders return packed ``MessageBatch``
objects (and the python-side inputs they were packed from) so GPU tests
can run the same batch through every writer, and CPU tests can check the
corpora's preconditions against the oracle alone.
"""
import datetime as dt
import random

from crawler_amd.ops import batch as B
from crawler_amd.ops import golden as G
from crawler_amd.ops.golden_batch import encode_batch

UTC = dt.timezone.utc
# the one timestamp the new writer/seen-set tests encode with (line
# lengths depend on it, so builders that target a length use it too)
NOW = dt.datetime(2026, 3, 4, 5, 6, 7, 890000, tzinfo=UTC)

# ---------------------------------------------------------------- fuzz corpus

WORDS = [
    "hello", "мир", "data", "🚀", "test", "канал", "🤯", "x" * 40,
    "a<b", "c&d", "e>f", 'q"r', "s\\t", "line\nbreak", "tab\there",
    "\u2028sep", "t.me/", "t.me/abcde", "https://t.me/fuzzchan",
    "@fuzz_name1", "t.me/joinchat/xyz", "plain", "…", "ñé",
    "t.me/abc", "word_with_underscores_here", "%%", "  ",
]


def rand_text(rng, max_words=14):
    return " ".join(rng.choice(WORDS) for _ in range(rng.randint(0, max_words)))


def utf16_len(s):
    return sum(2 if ord(c) >= 0x10000 else 1 for c in s)


def rand_entities(rng, text):
    """Well-formed entities at rune boundaries (TDLib guarantees this)."""
    ents = []
    if not text or rng.random() < 0.5:
        return ents
    for _ in range(rng.randint(1, 3)):
        # pick a rune-boundary slice
        i = rng.randint(0, len(text))
        j = rng.randint(i, min(len(text), i + 20))
        off16 = utf16_len(text[:i])
        len16 = utf16_len(text[i:j])
        etype = rng.choice(["mention", "url", "text_url"])
        url = ""
        if etype == "text_url":
            url = rng.choice([
                "https://t.me/fuzz_target1", "https://example.com/x",
                "t.me/abcd", "",
                # dead t.me before a live one (search must retry)
                "t.me/ %% t.me/deadlive1",
                # reserved first match ends the search
                "t.me/share t.me/after_rsv1",
            ])
        # occasionally overshoot the end (golden clamps)
        if rng.random() < 0.1:
            len16 += rng.randint(1, 5)
        ents.append(G.Entity(etype, off16, len16, url=url))
    return ents


def rand_message(rng, k):
    ct = rng.choice(B.CONTENT_TYPES)
    text = rand_text(rng)
    ft = G.FormattedText(text=text, entities=rand_entities(rng, text))
    reactions = {}
    for e in rng.sample(B.EMOJI_TABLE, rng.randint(0, 4)):
        reactions[e] = rng.randint(1, 10_000)
    return G.SynthMessage(
        chat_id=-1001000000000 - rng.randint(0, 10**6),
        msg_id=(k + 1) << 20,
        date=rng.randint(0, 2_000_000_000),
        content_type=ct,
        text=ft if ct == "messageText" else None,
        caption=ft if ct != "messageText" else None,
        views=rng.randint(0, 10**9),
        forwards=rng.randint(0, 10**6),
        reactions=reactions,
        media_album_id=rng.choice([0, 0, 0, rng.randint(1, 2**31 - 1)]),
        thumb_remote_id="AgAD%dt" % (k + 1) if rng.random() < 0.3 else "",
        video_remote_id="AgAD%dv" % (k + 1) if rng.random() < 0.2 else "",
        document_name=rand_text(rng, 2) if ct == "messageDocument" else "",
        emoji="🎉" if ct == "messageAnimatedEmoji" else "",
        poll_question=rand_text(rng, 3) if ct == "messagePoll" else "",
        giveaway_prize="premium" if ct == "messageGiveaway" else "",
        poster_handle=rng.choice(["", "user123", "фантом", 'we"ird\\']),
    )


def rand_comments(rng, n_msgs):
    out = []
    for _ in range(n_msgs):
        coms = []
        if rng.random() < 0.3:
            for _ in range(rng.randint(1, 3)):
                reacts = {}
                for e in rng.sample(B.EMOJI_TABLE, rng.randint(0, 2)):
                    reacts[e] = rng.randint(1, 500)
                coms.append((rand_text(rng, 5),
                             rng.choice(["u1", "коммент", ""]),
                             rng.randint(0, 10**6), rng.randint(0, 999),
                             reacts))
        out.append(coms)
    return out


def fuzz_corpus(seed, n):
    """(msgs, batch): n random messages with comments over 4 channels."""
    rng = random.Random(seed)
    msgs = [rand_message(rng, k) for k in range(n)]
    # reply_count must match packed comments for golden comment fetch
    comments = rand_comments(rng, n)
    for m, c in zip(msgs, comments):
        m.reply_count = len(c)
    channels = [B.ChannelRow(
        chat_id=-1001, username="fuzzchan%03d" % i,
        title=rand_text(rng, 3) or "t", member_count=rng.randint(0, 10**6),
        post_count=rng.randint(0, 10**5), total_views=rng.randint(0, 10**9),
    ) for i in range(4)]
    chan_of = [rng.randrange(4) for _ in range(n)]
    batch = B.pack(msgs, channels, chan_of, comments_of_msg=comments)
    return msgs, batch


def fuzz_batch(seed, n=120):
    """The fuzz corpus with comments and 4 channels."""
    return fuzz_corpus(seed, n)[1]


def median_cutoff(batch):
    """min_post_date at the batch's median date: filtered and kept lines
    interleave (dates are random per row)."""
    dates = sorted(int(d) for d in batch.meta["date"])
    return dt.datetime.fromtimestamp(dates[len(dates) // 2], UTC)


def future_cutoff(batch):
    """A min_post_date above every date in the batch."""
    return dt.datetime.fromtimestamp(
        max(int(d) for d in batch.meta["date"]) + 1, UTC)


# ------------------------------------------------------ handcrafted edge cases

EDGE_TEXTS = [
    # overlap/cursor semantics
    "t.me/abcdet.me/xyz12 tail",
    # 32-char cap
    "t.me/" + "a" + "b" * 40,
    # reserved + valid
    "t.me/joinchat/xx t.me/okchan1",
    # https prefix + dup
    "https://t.me/dupdup1 t.me/dupdup1",
    # unicode + escapes + U+2028
    'привет "мир" <>&\n\u2028 t.me/unichan1 🚀',
    # no links
    "just plain text",
    # mention entity with cyrillic prefix
    "канал @mention_chan тут",
]


def edge_batch():
    """(texts, batch): adversarial messages through the real packer."""
    msgs = []
    texts = list(EDGE_TEXTS)
    for k, t in enumerate(texts):
        ents = []
        if "@mention_chan" in t:
            off = t.index("@")
            ents.append(G.Entity("mention", off, len("@mention_chan")))
        msgs.append(G.SynthMessage(
            chat_id=-100123, msg_id=(k + 1) << 20, date=1_700_000_000 + k,
            content_type="messageText",
            text=G.FormattedText(text=t, entities=ents),
            views=k * 10, forwards=k, reactions={"👍": k + 1},
            poster_handle=f"user{k:04d}",
        ))
    ch = [B.ChannelRow(chat_id=-100123, username="edgechan1",
                       title='Edge "Chan" <&>', member_count=5,
                       post_count=len(msgs), total_views=100)]
    return texts, B.pack(msgs, ch, [0] * len(msgs))


# ------------------------------------------------ SWAR block-boundary escapes

def swar_texts():
    """Adversarial placement of escape bytes around the measure pass's
    256-byte SWAR blocks (common.h esc fast path): U+2028/29 leaders at
    block edges, specials at every lane-word position, long clean runs."""
    U2028 = "\u2028"
    U2029 = "\u2029"
    texts = []
    # E2-leader at byte offsets straddling the 256-byte block boundary.
    # description starts at the raw text start, so byte index within the
    # field == byte index within the python string's utf-8 encoding.
    for lead in (253, 254, 255, 256, 257):
        t = "a" * lead + U2028 + "b" * 300
        texts.append(t)
        texts.append("a" * lead + U2029 + "b" * 300)
    # special byte at each position of the first lane word
    for pos in (0, 1, 2, 3, 63, 64, 127, 255, 256, 511):
        t = ("x" * pos) + '"' + ("y" * 400)
        texts.append(t)
    # a control byte deep in an otherwise clean 1KB run
    texts.append("c" * 700 + "\x07" + "d" * 300)
    # fully clean 1KB (pure fast path), clean multiple-of-256
    texts.append("e" * 1024)
    texts.append("f" * 512)
    # dirty first block then long clean tail (fast path must re-engage)
    texts.append("<&>" + "g" * 900)
    # non-ascii high bytes that are NOT E2 sequences (must stay clean-ish)
    texts.append("п" * 400)   # 0xD0 0xBF pairs
    # E2 that is NOT a U+2028/29 (e.g. '…' U+2026 = E2 80 A6)
    texts.append("h" * 250 + "…" + "i" * 300)
    return texts


def swar_batch():
    """(texts, batch) for :func:`swar_texts`."""
    texts = swar_texts()
    msgs = []
    for k, t in enumerate(texts):
        msgs.append(G.SynthMessage(
            chat_id=-100555, msg_id=(k + 1) << 20,
            date=1_700_100_000 + k, content_type="messageText",
            text=G.FormattedText(text=t),
            views=k, forwards=0, poster_handle=f"user{k:04d}",
        ))
    ch = [B.ChannelRow(chat_id=-100555, username="swarchan1",
                       title="SWAR", member_count=3,
                       post_count=len(msgs), total_views=9)]
    return texts, B.pack(msgs, ch, [0] * len(msgs))


# ------------------------------------------------------------- LDS ladder

LDS_LINE_BYTES = 3072   # parse_encode.hip: write_lds_kernel's per-wave buffer
_ESC_UNIT = '"<\n\u2028'    # 6 raw bytes -> 16 escaped bytes


def _ladder_pack(texts):
    msgs = [G.SynthMessage(
        chat_id=-100888, msg_id=(k + 1) << 20, date=1_700_200_000 + k,
        content_type="messageText", text=G.FormattedText(text=t),
        views=100 + k, forwards=k % 7, poster_handle="poster%02d" % (k % 100),
    ) for k, t in enumerate(texts)]
    ch = [B.ChannelRow(chat_id=-100888, username="ldsladder", title="L",
                       member_count=7, post_count=len(msgs), total_views=70)]
    return B.pack(msgs, ch, [0] * len(msgs))


# target oracle line length per row (None = text given verbatim)
_LADDER_PLAN = [
    (40, None), (3070, None), (41, None), (3071, None), (42, None),
    (3072, None), (43, None), (3073, None), (3074, None),
    # cross LDS_LINE_BYTES only after escaping
    (None, _ESC_UNIT * 100),
    (None, "a" * 700 + _ESC_UNIT * 40 + "tail"),
    (44, None), (3072, None), (3071, None), (3070, None),
]


def lds_ladder():
    """One batch of clean-ASCII messageText posts whose oracle line
    lengths cover 3070..3074 (straddling ``LDS_LINE_BYTES``), two lines
    that exceed it only after escaping, and line starts in all four
    residues mod 4 (the funnel-shift copy's head/tail cases).

    Text lengths are derived from the oracle: a probe batch with 1-byte
    texts gives each row's fixed overhead (clean ASCII adds one output
    byte per text byte)."""
    probe = _ladder_pack(["x" if t is None else t for _, t in _LADDER_PLAN])
    base, _ = encode_batch(probe, now=NOW)
    texts = []
    for (target, text), line in zip(_LADDER_PLAN, base):
        if text is not None:
            texts.append(text)
        elif target < 1000:          # short filler: text length as given
            texts.append("s" * target)
        else:
            texts.append("k" * (target - (len(line) - 1)))
    return _ladder_pack(texts)


def lds_ladder_escape_rows():
    """Row indices of the two escape-crossing lines in lds_ladder()."""
    return [i for i, (_, t) in enumerate(_LADDER_PLAN) if t is not None]


# ----------------------------------------------------------- stage ladder

_STAGE_USER = "stage_chan_01"
_STAGE_TITLE = 'Stage "T" <&>\n\u2028я'
_STAGE_POSTER = 'we"ird\\'


def _stage_text(nbytes):
    """Exactly ``nbytes`` UTF-8 bytes: 8 distinct valid t.me links, some
    escapes and multi-byte runes, then clean ASCII padding."""
    head = " ".join("t.me/stagelink%02d" % j for j in range(8))
    head += ' я"<\n\u2028> 🚀 '
    pad = nbytes - len(head.encode("utf-8"))
    assert pad >= 0, "stage budget too small for the link header"
    return head + "p" * pad


def _stage_batch(field_bytes):
    long_text = _stage_text(field_bytes)
    doc_name = 'doc "n" <&> ' + "d" * (field_bytes - 12)
    msgs = [
        G.SynthMessage(
            chat_id=-100999, msg_id=1 << 20, date=1_700_300_000,
            content_type="messageText",
            text=G.FormattedText(text=long_text),
            views=12345, forwards=67,
            reactions={e: 10 + j for j, e in enumerate(B.EMOJI_TABLE)},
            poster_handle=_STAGE_POSTER,
        ),
        G.SynthMessage(
            chat_id=-100999, msg_id=2 << 20, date=1_700_300_001,
            content_type="messageDocument",
            caption=G.FormattedText(text="see t.me/stagedoc01"),
            document_name=doc_name, views=5, forwards=1,
            reactions={"🔥": 3}, poster_handle=_STAGE_POSTER,
        ),
        G.SynthMessage(
            chat_id=-100999, msg_id=3 << 20, date=1_700_300_002,
            content_type="messageText",
            text=G.FormattedText(text="short t.me/stageshort1"),
            views=1, forwards=0, poster_handle="u3",
        ),
    ]
    ch = [B.ChannelRow(chat_id=-100999, username=_STAGE_USER,
                       title=_STAGE_TITLE, member_count=11,
                       post_count=len(msgs), total_views=999)]
    return B.pack(msgs, ch, [0] * len(msgs))


def stage_ladder(budget, fixed):
    """(at, over): two batches whose staged-writer gate arithmetic
    ``fixed + max(text, aux) + poster + user + title`` lands exactly on
    ``budget`` and on ``budget + 1``. Row 0 carries 8 distinct links and
    all 10 reactions at the maximum text length; row 1 takes its
    description from ``aux`` (a document name) at the same length."""
    rest = (len(_STAGE_POSTER.encode("utf-8"))
            + len(_STAGE_USER.encode("utf-8"))
            + len(_STAGE_TITLE.encode("utf-8")))
    field = budget - fixed - rest
    return _stage_batch(field), _stage_batch(field + 1)


# --------------------------------------------------------- seen-set hashes

_U64 = (1 << 64) - 1


def home_slot_hashes(home, count, slots_log2, salt=0):
    """``count`` distinct 64-bit hashes whose home slot (h & (slots-1))
    is ``home``; high bits are scrambled so some have the top bit set."""
    mask = (1 << slots_log2) - 1
    out = []
    for j in range(count):
        hi = ((j + 1 + salt) * 0x9E3779B97F4A7C15) & _U64 & ~mask
        out.append(hi | home)
    return out


def wrap_chain_hashes():
    """40 hashes homed at the last slot of a 64-slot table (the probe
    sequence must wrap to slot 0) plus 8 homed at slot 0 (pushed along
    by the wrapped chain)."""
    return home_slot_hashes(63, 40, 6), home_slot_hashes(0, 8, 6, salt=1000)


def bloom_hashes():
    """Two claim rounds for the bloom check: includes h = 0, hashes with
    the top bit set, and a pair sharing their low bloom probe."""
    first = [0, 1 << 63, _U64, 0x8000000000000401, 0x0000000100000401,
             0x123456789ABCDEF0, 0xFEDCBA9876543210, 5, 1023 | (1023 << 32)]
    second = [0x0F0F0F0F0F0F0F0F, 0x8000000000000000 | 777, 5,
              0x00000200_00000100]
    return first, second


def dup_hashes():
    """16 distinct hashes, to be tiled over 2048 link slots."""
    return [((j + 1) * 0xD6E8FEB86659FD93) & _U64 | 2 for j in range(16)]


# ------------------------------------------------------- YouTube encoder
#
# Hand-made rows for csrc/yt_encode.hip, packed with pack_videos; one
# small generator per concern. Every string is valid UTF-8 (the oracle
# decodes strictly) and none holds byte 0xA5, the poison the GPU tests
# pre-fill the output with. pack_videos lays the pool out as
# [id | title | description] per row, then the channel table, so row
# i's description is followed directly by row i+1's 11-byte id.

YT_POISON = 0xA5
YT_MAX_VIEWS = 2 ** 53      # YouTubeBatch: views is valid in 0 .. 2**53
_YT_EPOCH = dt.datetime(1970, 1, 1, tzinfo=UTC)


def _yt_time(secs):
    return _YT_EPOCH + dt.timedelta(seconds=secs)


def _yt_video(k, title="t", desc="", vid=None, published=None, views=0,
              likes=0, comments=0, duration="PT1M1S", language="en"):
    from crawler_amd.youtube.synth import YouTubeVideo

    return YouTubeVideo(
        id=vid or "v%04d-abcde" % k, channel_id="", title=title,
        description=desc,
        published_at=_yt_time(1_700_000_000 + k if published is None
                              else published),
        view_count=views, like_count=likes, comment_count=comments,
        duration=duration, language=language)


def _yt_channel(k, title=None, desc="about", country="US", subs=0,
                videos=0, views=0, published=1_600_000_000):
    from crawler_amd.youtube.synth import YouTubeChannel

    return YouTubeChannel(
        id="UC%022d" % k, title="Chan %d" % k if title is None else title,
        description=desc, subscriber_count=subs, video_count=videos,
        view_count=views, country=country, published_at=_yt_time(published))


def _yt_pack(videos, channels=None, channel_of=None, label="yt-matrix"):
    from crawler_amd.youtube.batch import pack_videos

    if channels is None:
        channels, channel_of = [_yt_channel(0)], [0] * len(videos)
    return pack_videos(videos, channels, channel_of, crawl_label=label)


def _yt_many_urls(count, tag):
    return " ".join("https://m%s.example/p%02d" % (tag, j)
                    for j in range(count))


_YT_TRIM = ",.;:!?()'\""
_YT_STOPS = "\t\n\f\r <>\""

# (description, id of the row or None). pack_videos puts row i+1's id
# right behind row i's description, so an id is the bait a scanner that
# reads past desc_len would pick up.
_YT_URL_ROWS = [
    # bare scheme: before a space, before '<', at end of text
    ("see http:// x", None),
    ("http://<b", None),
    ("https:// and https://<b> and https://\"q\"", None),
    ("bare at end http://", None),
    ("plain text", "x.example/y"),       # would complete the bare scheme
    ("bare at end https://", None),
    ("both http://a.example/1 https://b.example/2", None),
    ("HTTP://a Http://b hTTps://c", None),
    ("hthttp://a", None),
    ("httphttp://a", None),
    ("httpshttps://a httpss://b http:/c http//d", None),
    ("http://a<http://b", None),
    ("https://a.b/c).,", None),
    ("(https://a.b/d?!;:')", None),
    ("http://.", None),
    ("http://.,; https://:", None),
    # every trim byte alone ('"' also stops the URL)
    (" ".join("x https://t%d.example/c%s y" % (j, c)
              for j, c in enumerate(_YT_TRIM)), None),
    # duplicates that differ only by trimmed punctuation
    ("http://dup.example/x, http://dup.example/x. (http://dup.example/x)"
     " http://dup.example/x", None),
    # equal length, last byte differs; then a true duplicate of the first
    ("http://same.len/a http://same.len/b http://same.len/a"
     " http://same.len/c http://same.len/b", None),
    # bytes that CONTINUE a URL under the byte-level stop set
    ("http://a\x01b c", None),
    ("http://a\x0bb c", None),
    ("http://a\x7fb c", None),
    ("http://a\u00a0b c", None),
    ("http://a\u2028b c", None),
    ("http://a\x1cb\x1d\x1e\x1f\u0085\u3000c d", None),
    # each real stop byte
    (" ".join("http://s%d%stop" % (j, c)
              for j, c in enumerate(_YT_STOPS)), None),
    # a URL that needs JSON escaping
    ("https://e.sc/?a=1&b=2\\c&d https://e.sc/?a=1&b=2\\c&d.", None),
    (_yt_many_urls(9, "a"), None),
    (_yt_many_urls(10, "b"), None),
    (_yt_many_urls(40, "c"), None),
    # 12 URLs of which 4 repeat earlier ones
    (" ".join(["https://d.example/%d" % j for j in range(8)]
              + ["https://d.example/3,", "https://d.example/0",
                 "https://d.example/7.", "https://d.example/5"]), None),
    # 12 URLs, 9 distinct: a repeat of the 9th, and of the 1st after it
    (" ".join(["https://g.example/%d" % j for j in range(9)]
              + ["https://g.example/8", "https://g.example/0.",
                 "https://g.example/8,"]), None),
    # shorter than the shortest match, and empty
    ("http:/", None),
    ("h", None),
    ("", None),
    # a URL ending exactly at desc_len, the next row's id continuing it
    ("end http://tail.example/p", None),
    ("after the bait", "ath/http://"),
    # "htt" at the very end, the next row's id completing the scheme
    ("see htt", None),
    ("after the second bait", "p://abc.de/"),
    # equal length AND equal last byte, different in the middle; then
    # true duplicates of both
    ("http://mid.a/x http://mid.b/x, http://mid.a/x http://mid.b/x", None),
]


def yt_url_edges():
    """Descriptions for the URL scanner: bare schemes, scheme
    look-alikes, trimming, dedup, the byte-level stop set, more than 8
    URLs, escapes, and text cut off by desc_len with URL-like bytes
    right behind it."""
    return _yt_pack([_yt_video(k, title="url %d" % k, desc=d, vid=vid)
                     for k, (d, vid) in enumerate(_YT_URL_ROWS)])


def yt_sanitize_edges():
    """Titles for sanitized(): run collapsing and the 80-byte cap."""
    titles = [
        "", "!!!", "!", "  lead", "trail  ", "in  ner   runs",
        "\u00e9\u00e9\u00e9", "a\U0001F680b",
        "\u00e9\u00e9\u00e9\U0001F680\u00e9x\u00e9", "keep.dots-and_under",
        "..--__", "s" * 79 + "!!y", "s" * 79 + "y", "s" * 79 + "!",
        "s" * 80 + "more", "s" * 80 + "!!", "s" * 80, "a!" * 60,
        "!a" * 60, "!" * 200 + "x", "\u00e9" * 200 + "x",
        "w" * 78 + "\U0001F680\U0001F680zz",
    ]
    return _yt_pack([_yt_video(k, title=t, desc="d%d" % k)
                     for k, t in enumerate(titles)])


YT_ESC_LENGTHS = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 259, 260,
                  511, 512, 513, 1030]
_YT_SPECIALS = ['"', "\\", "\n", "<", "&", "\x01"]


def _yt_esc_strings():
    """The ladder's strings: each length clean, then with ONE special
    byte at the first, the last, and every 256-byte block-boundary-1 /
    block-boundary position below the length. The special cycles through
    the six escape classes from string to string; at length 513 all six
    sit at both sides of the first block boundary. Then U+2028 at every
    split over a block start, and an E2-led non-2028 character there."""
    out = []
    k = 0
    for n in YT_ESC_LENGTHS:
        out.append("a" * n)
        pos = {0, n - 1} | {b + d for b in range(256, n + 1, 256)
                            for d in (-1, 0)}
        for p in sorted(q for q in pos if 0 <= q < n):
            sp = _YT_SPECIALS[k % 6]
            k += 1
            out.append("b" * p + sp + "c" * (n - p - 1))
    for sp in _YT_SPECIALS:
        for p in (255, 256):
            out.append("d" * p + sp + "e" * (513 - p - 1))
    for lead in (253, 254, 255, 256, 509, 510, 511, 512):
        out.append("f" * lead + "\u2028" + "g" * 300)
    for lead in (253, 254, 255, 256):
        out.append("h" * lead + "\u2014" + "i" * 300)
    return out + swar_texts()


def _yt_esc_batch(strings, label):
    """Row i: title strings[i], description strings[i+1]; one channel
    per 4 rows carrying three more of them (title, description,
    country)."""
    m = len(strings)
    videos = [_yt_video(k, title=strings[k], desc=strings[(k + 1) % m])
              for k in range(m)]
    channels = [_yt_channel(j, title=strings[(4 * j) % m],
                            desc=strings[(4 * j + 1) % m],
                            country=strings[(4 * j + 2) % m])
                for j in range((m + 3) // 4)]
    return _yt_pack(videos, channels, [k // 4 for k in range(m)], label)


YT_LABELS = ["", 'la"b\\el <&>\n\u2028\u00e9',
             "l" * 255 + '"' + "m" * 44]


def yt_esc_ladder():
    """List of batches (<= 40 rows each) over :func:`_yt_esc_strings`,
    the same strings in title, description, channel title, channel
    description and country; then one small batch per crawl_label in
    YT_LABELS (empty, escaped, 300 bytes)."""
    strings = _yt_esc_strings()
    out = [_yt_esc_batch(strings[i:i + 40], "esc-%d" % i)
           for i in range(0, len(strings), 40)]
    few = ["plain", 'q"<\n', "n" * 300]
    out += [_yt_esc_batch(few, label) for label in YT_LABELS]
    return out


_YT_BIG = sorted({0, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1}
                 | {10 ** k - d for k in range(1, 16) for d in (0, 1)})
YT_DATES = [-62135596800, -1, 0, 951782400, 4107542400, 68169600,
            253402300799]
_YT_DURATIONS = ["P0D", "PT0S", "PT1S", "PT%dS" % (2 ** 31 - 1)]
_I32_MAX = 2 ** 31 - 1


def yt_number_edges():
    """Counters at every decimal-length step and around 2**32 (the
    32/64-bit split of u64()), the int32 and int64 maxima, engagement
    past int32, durations and dates at the edges of their domains."""
    views = _YT_BIG + [2 ** 53 - 1, 2 ** 53]
    ch_big = _YT_BIG + [2 ** 63 - 1]
    videos, channels = [], []
    for k, v in enumerate(views):
        likes = _I32_MAX if k % 3 == 0 else 0
        comments = _I32_MAX if k % 3 != 1 else 0   # k % 3 == 0: both max
        videos.append(_yt_video(
            k, views=v, likes=likes, comments=comments,
            duration=_YT_DURATIONS[k % 4], language=("en", "ru")[k % 2],
            published=YT_DATES[k % 7], title="n%d" % k, desc="v=%d" % v))
    for j, s in enumerate(ch_big):
        channels.append(_yt_channel(
            j, subs=s, views=ch_big[(j + 5) % len(ch_big)],
            videos=_I32_MAX if j % 2 else 0,
            published=YT_DATES[(j + 3) % 7]))
    return _yt_pack(videos, channels,
                    [k % len(channels) for k in range(len(videos))])


YT_SHAPE_NS = [1, 2, 3, 5, 7, 9]


def yt_shape_batches():
    """{n: batch} for n in YT_SHAPE_NS: the first n of nine rows whose
    line lengths differ widely; rows share channels, and the channel
    table's order is not the rows' first-appearance order."""
    descs = ["", "http://s.example/1 " * 30, "short", "x" * 900 + "<&>",
             _yt_many_urls(12, "s"), "d", "\u2028" * 90, "e" * 257,
             "last http://s.example/z."]
    titles = ["t", "T" * 300, "", "a!" * 50, "mid", "\u00e9" * 120,
              "t6", "s" * 81, "nine"]
    channel_of = [3, 0, 3, 1, 0, 2, 3, 1, 0]
    channels = [_yt_channel(j, title="C%d " % j + "z" * (70 * j),
                            desc="about " * (5 * (3 - j)),
                            country=("US", "", "DE", "")[j], subs=10 ** j)
                for j in range(4)]
    videos = [_yt_video(k, title=titles[k], desc=descs[k], views=7 ** k,
                        likes=k, comments=2 * k) for k in range(9)]
    return {n: _yt_pack(videos[:n], channels, channel_of[:n])
            for n in YT_SHAPE_NS}


def yt_corpora():
    """{name: batch}: every YouTube corpus above, one entry per batch."""
    out = {"url": yt_url_edges(), "sanitize": yt_sanitize_edges(),
           "numbers": yt_number_edges()}
    for j, b in enumerate(yt_esc_ladder()):
        out["esc%d" % j] = b
    for n, b in yt_shape_batches().items():
        out["shape%d" % n] = b
    return out


def encode_yt_lines(batch):
    """Oracle lines of a YouTube batch at NOW."""
    from crawler_amd.youtube.batch import encode_yt_batch

    return encode_yt_batch(batch, now=NOW)


# ------------------------------------------------- shared GPU-test helpers

def assert_batches_equal(cpu_b, dev_b):
    """Every field of two MessageBatch objects: same dtype, shape, bits."""
    import dataclasses

    import torch

    def same(name, a, b):
        b = b.cpu()
        assert a.dtype == b.dtype, f"{name}: {a.dtype} vs {b.dtype}"
        assert a.shape == b.shape, f"{name}: {a.shape} vs {b.shape}"
        assert torch.equal(a, b), (
            f"{name} differs at "
            f"{(a != b).nonzero()[:5].flatten().tolist()}"
        )

    for f in dataclasses.fields(cpu_b):
        a = getattr(cpu_b, f.name)
        b = getattr(dev_b, f.name)
        if isinstance(a, dict):
            assert sorted(a) == sorted(b), f"{f.name} keys differ"
            for k in a:
                same(f"{f.name}[{k}]", a[k], b[k])
        elif isinstance(a, torch.Tensor):
            same(f.name, a, b)
        else:
            assert a == b, f"{f.name}: {a} != {b}"


def force_grid_one(monkeypatch, names):
    """Patch ``gpu._call`` so that the entry points in ``names`` launch
    one block: the grid is their last positional argument. Returns the
    list the patched calls are recorded in."""
    from crawler_amd.ops import gpu

    real, seen = gpu._call, []

    def call(name, *args, **kw):
        if name in names:
            assert isinstance(args[-1], int) and args[-1] >= 1, name
            args = args[:-1] + (1,)
            seen.append(name)
        return real(name, *args, **kw)

    monkeypatch.setattr(gpu, "_call", call)
    return seen


def forbid_launches(monkeypatch):
    """Patch ``gpu._call`` to fail: the code under test must not launch."""
    from crawler_amd.ops import gpu

    def call(name, *args, **kw):
        raise AssertionError(f"unexpected launch of {name}")

    monkeypatch.setattr(gpu, "_call", call)


# ----------------------------------------------------- feed generator matrix

FEED_SHAPES = [(1, 1), (1, 3), (2, 1), (3, 5), (5, 257), (1, 1025)]
FEED_BIG = (5, 7000)          # 35 000 messages > 8192 blocks x 4 waves
FEED_FORCED = [(3, 5), (5, 257)]
# the forced-grid runs: one block of 256 threads has to stride over the
# comments too, so every second message carries up to three
FEED_FORCED_CFG = dict(seed=79, universe=100_000, comment_rate=0.5,
                       max_comments_per_post=3)


def feed_cases():
    """[(name, FeedConfig keywords, channel ids, posts per channel)]: the
    matrix both builders run over."""
    base = dict(seed=77, universe=100_000)
    cases = []
    for K, P in FEED_SHAPES + [FEED_BIG]:
        cases.append(("shape-%dx%d" % (K, P), base, list(range(10, 10 + K)),
                      P))
    cases.append(("ids-unsorted", base, [905, 3, 77_000, 12, 4], 33))
    cases.append(("ids-duplicate", base, [7, 7, 3], 33))
    cases.append(("ids-extremes", dict(seed=77, universe=1000),
                  [0, 999, 1000, 2 ** 40], 33))
    for rate in (0.0, 0.001, 0.5, 1.0):
        for mc in (1, 3, 50):
            cases.append(("rate-%s-max-%d" % (rate, mc),
                          dict(base, comment_rate=rate,
                               max_comments_per_post=mc), [5, 6, 9], 40))
    cases.append(("rate-1.0-one-post",
                  dict(base, comment_rate=1.0), [5, 6, 9], 1))
    for universe in (1, 2, 10 ** 10 - 1):
        cases.append(("universe-%d" % universe,
                      dict(seed=77, universe=universe), [1, 8], 50))
    for seed in (0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1):
        cases.append(("seed-%d" % seed, dict(seed=seed, universe=100_000),
                      [1, 8], 50))
    # dates 2**31 - 100 + 7 * p (+ 0..29): the first posts stay below
    # 2**31, the later ones wrap through int32
    cases.append(("dates-wrap", dict(base, base_date=2 ** 31 - 100,
                                     date_step=7), [1, 8], 50))
    return cases


def feed_entity_templates():
    """A template set whose messages carry 0, 1, 4 and 70 entity rows
    (the standard set stops at one): rows with and without a url inside
    one message, and more rows than a wave has lanes."""
    from crawler_amd.feed.synth import Template

    return [
        Template(name="none", content_type="messageText",
                 text="без ссылок 🚀"),
        Template(name="one", content_type="messageText",
                 text="спасибо @{U} за наводку",
                 entity_specs=[("mention", 0)]),
        Template(name="four", content_type="messageText", weight=2.0,
                 text=("спасибо @{U} 🙏 источник: https://t.me/{U} — "
                       "click here и ещё @{U}"),
                 entity_specs=[("mention", 0), ("url", 1), ("text_url", 0),
                               ("mention", 2)]),
        Template(name="seventy", content_type="messagePhoto",
                 text="@{U} " * 70, has_thumb=True,
                 entity_specs=[("mention", j) for j in range(70)]),
    ]


FEED_ENTITY_CASE = (dict(seed=80, universe=100_000, comment_rate=0.5),
                    [3, 1, 4], 21)


# ------------------------------------------------------- t.me HTML corpora

HTML_VALID = ("valid", "")
HTML_NOT_CHANNEL = ("not_channel", "not_supergroup")
HTML_NOT_FOUND = ("invalid", "not_found")
HTML_UNRECOGNIZED = ("invalid", "unrecognized")

_CONTACT = b"<title>Telegram: Contact @a</title>"
_ROBOTS = b'<meta name="robots" content="noindex">'

# documents on which the kernel was read to disagree with the oracle, with
# the oracle's answer
HTML_TABLE_ROWS = [
    (b"<TITLE>Telegram: View @a</TITLE>", HTML_VALID),
    (b"<title>\x0cView @a</title>", HTML_VALID),
    (b"<title>Foo</title x>Telegram: View @a</title>", HTML_VALID),
    (_CONTACT + b'<META NAME="ROBOTS" CONTENT="NOINDEX">', HTML_NOT_FOUND),
    (_CONTACT + b'<meta name="robots\' content=\'noindex\'>',
     HTML_NOT_FOUND),
    (_CONTACT + b'<meta name=\'robots\' content="noindex" name="robots">',
     HTML_NOT_FOUND),
    (_CONTACT + b'<metaname="robots" content="noindex">', HTML_NOT_CHANNEL),
    (_CONTACT + b'<meta name="robots"noindex>', HTML_NOT_CHANNEL),
]

HTML_RULES = [b"View @", b"Telegram: View @", b"Contact @",
              b"Telegram: Contact @", b"Telegram Messenger"]


def html_rule_docs():
    """Each title rule at the start, in the middle and at the end of the
    title, bare and behind every strippable byte; the title tag's forms;
    the noindex forms."""
    docs = []
    for rule in HTML_RULES:
        for title in (rule + b"a tail", b"head " + rule + b"a tail",
                      b"head " + rule, rule,
                      b" \t\n\r\x0b\x0c" + rule + b"a \x0c\x0b\r\n\t ",
                      b"\x0b" + rule + b"a", b"\xa0" + rule + b"a",
                      b"\x1c" + rule + b"a", rule[:-1], rule.lower(),
                      rule.upper()):
            docs.append(b"<html><title>" + title + b"</title>" + _ROBOTS)
            docs.append(b"<title>" + title + b"</title>")
    v = b"View @a"
    docs += [
        b"<title lang=en>" + v + b"</title>",
        b"<titlex>" + v + b"</title>",
        b"<TiTlE LANG='en'>" + v + b"</tItLe>",
        b"<title " + v,                              # no '>' at all
        b"<title " + v + b"</title>",                # its only '>' closes
        b"<title " + v + b"</title></title>",
        b"<title>" + v,                              # no close tag
        b"<title>" + v + b"</title",
        b"<title>" + v + b"< /title>",
        b"<title></title>",
        b"<title> \t\n\r\x0b\x0c</title>",
        b"<title>" + v + b"</title><title>Telegram Messenger</title>",
        b"<title>Telegram Messenger</title><title>" + v + b"</title>",
        b"<title>x</title><title>" + v + b"</title>",
        b"<title><title>" + v + b"</title>",
        b"<titl>" + v + b"</title>",
        b"< title>" + v + b"</title>",
        b"</title><title>" + v + b"</title>",
        b"<title>Telegram Messenger</title>" + _ROBOTS,
        b"<html><head></head><body>no title</body></html>",
        b"<", b">", b"<title", b"<title>", b"</title>", b"\x00",
    ]
    c = _CONTACT
    docs += [
        c,
        c + _ROBOTS,
        _ROBOTS + c,                                  # meta before the title
        c + b'<meta content="noindex" name="robots">',   # only before name=
        c + b'<meta name="robots"><meta content="noindex">',  # later tag
        c + b'<meta name="robots" content="index">noindex',   # body text
        c + b'<meta name="robots" content="index"> noindex <p>',
        c + b'<meta name="robots" content="noindex"',    # unterminated
        c + b'<meta name="robots" content="noinde',
        c + b'<meta name="robots" content="noindex',
        c + b"<meta",
        c + b"<meta ",
        c + b'<meta name="robots"',
        c + b'<meta name="robots" ',
        c + (b'<meta name="description" content="noindex">'
             b'<meta name="robots" content="all">'
             b'<meta name="viewport">' + _ROBOTS),    # only the last matches
        c + (b'<meta name="robots" content="all">') * 3,
        c + b"<meta" + _ROBOTS,                       # <meta<meta ...
        c + b"<meta><meta><meta" + _ROBOTS,
        c + b'<meta x name="robots" y noindex>',
        c + b'<meta name="robots" noindex>',
        c + b'<meta name="robots"_noindex>',
        c + b'<meta name="robots" NoInDeX>',
        c + b"<mEtA nAmE='rObOtS\" content=noindex>",
        c + b'<meta name=robots content="noindex">',   # no quotes
        c + b'<meta name="robots content="noindex">',
        c + b'<meta name= "robots" content="noindex">',
        c + b'<meta name="robot" name="robots" content="noindex">',
        c + b'<meta name="robots" content="no index">',
        c + b'<meta\nname="robots"\ncontent="noindex"\n>',
        c + b'<link name="robots" content="noindex">',
        c + b'<meta name="robots"> <meta noindex>',
        c + b'<meta name="robots" content=">" noindex>',
        b"<title>Contact @a</title>" + _ROBOTS,
        b"<title>Contact @a</title>",
    ]
    return docs


HTML_EDGE_OFFSETS = list(range(58, 71)) + list(range(122, 135))


def html_window_edges():
    """[(kind, offset, doc, oracle answer)]: each pattern the kernel
    searches for, starting ``offset`` bytes into the range it is searched
    in (a 64-lane window walks that range). A missed pattern changes the
    answer: valid becomes unrecognized, not_found becomes not_channel."""
    v = b"View @a"
    out = []
    for off in HTML_EDGE_OFFSETS:
        pad = b"x" * off
        out += [
            # range: the whole body
            ("title_open", off, pad + b"<title>" + v + b"</title>",
             HTML_VALID),
            # range: from behind '<title'
            ("title_gt", off, b"<title" + b" " * off + b">" + v
             + b"</title>", HTML_VALID),
            # range: from behind the tag's '>'
            ("title_close", off, b"<title>" + v + b"x" * (off - len(v))
             + b"</title>", HTML_VALID),
            # range: the whole body (the first <meta)
            ("meta_first", off, b"<title>Contact @a</title>"
             + b"x" * (off - 25) + _ROBOTS, HTML_NOT_FOUND),
            # range: from behind the previous '<meta'
            ("meta_next", off, b"<meta>" + pad[1:] + _ROBOTS + _CONTACT,
             HTML_NOT_FOUND),
            # range: from m + 6
            ("name", off, _CONTACT + b"<meta " + b"a" * off
             + b'name="robots" content="noindex">', HTML_NOT_FOUND),
            # range: from r + 14
            ("noindex", off, _CONTACT + b'<meta name="robots"_'
             + b"a" * off + b"noindex>", HTML_NOT_FOUND),
        ]
    return out


def html_short_ranges():
    """Search ranges shorter than the pattern searched in them."""
    c = _CONTACT
    return [
        b"", b"<", b"<titl", b"<title", b"<title>",
        b"<title>V</title>", b"<title>View </title>",
        b"<title>View @</title>", b"<title>Contact </title>",
        b"<title>Telegram Messenge</title>",
        b"<title>View @a</titl", b"<title>View @a</title",
        b"<title>View @a<", b"<title>View @a",
        c + b"<", c + b"<met", c + b"<meta", c + b"<meta n",
        c + b"<meta name=", c + b'<meta name="robots',
        c + b'<meta name="robots"', c + b'<meta name="robots" ',
        c + b'<meta name="robots" n', c + b'<meta name="robots" noinde',
        c + b'<meta name="robots" noindex',
        c + b'<meta name="robots">noindex',
    ]


HTML_CAP = 64 * 1024


def html_cap_docs():
    """[(doc, oracle answer)] around the 64 KiB body cap."""
    def titled(total):
        # '</title>' ends at byte ``total``
        body = b"<title>View @a"
        return body + b"x" * (total - len(body) - 8) + b"</title>"

    def meta_ending_at(end, tail):
        head = _CONTACT
        meta = b'<meta name="robots" content="noindex'
        return head + b"x" * (end - len(head) - len(meta)) + meta + tail

    behind = _CONTACT + b"x" * (HTML_CAP - len(_CONTACT)) + _ROBOTS
    behind += b"y" * (70_000 - len(behind))
    return [
        (titled(HTML_CAP), HTML_VALID),
        (titled(HTML_CAP + 1), HTML_UNRECOGNIZED),
        (titled(HTML_CAP + 1) + b"<title>View @b</title>",
         HTML_UNRECOGNIZED),
        (behind, HTML_NOT_CHANNEL),
        # 'noindex' ends at the cap, with the tag's '>' behind it
        (meta_ending_at(HTML_CAP, b'">'), HTML_NOT_FOUND),
        # ... and one byte later, so the cap cuts its 'x'
        (meta_ending_at(HTML_CAP + 1, b'">'), HTML_NOT_CHANNEL),
    ]


def html_packing_docs():
    """Documents to classify back to back, in this order: document 2j ends
    1..8 bytes short of completing '</title>' (or 'noindex'), and document
    2j+1 starts with the missing bytes. Reading past a document's end
    turns unrecognized into valid, and not_channel into not_found."""
    docs = []
    full = b"<title>View @a</title>"
    for cut in range(1, 9):
        docs.append(full[:-cut])
        docs.append(full[-cut:] + b"<title>Telegram Messenger</title>")
    full = _CONTACT + b'<meta name="robots" content="noindex'
    for cut in range(1, 8):
        docs.append(full[:-cut])
        docs.append(full[-cut:] + b'"><title>View @b</title>')
    return docs


_HTML_TOKENS = [
    b"<title", b"<TITLE", b">", b"</title>", b"</TITLE>", b"</title",
    b"View @", b"Telegram: View @", b"Contact @", b"Telegram: Contact @",
    b"Telegram Messenger", b"<meta", b"<META", b" ", b"\x0c", b"\n",
    b'name="robots"', b"name='robots'", b'NAME="Robots\'', b"name=",
    b"robots", b'"', b"'", b"noindex", b"NOINDEX", b"noinde", b"x", b"a",
    b"<", b"=", b"content=", b"x" * 61,
]


def html_fuzz_docs(seed, n):
    """Token soup over the pieces the two regexes look for."""
    rng = random.Random(seed)
    docs = []
    for _ in range(n):
        head = rng.choice([b"", b"<title>Telegram: Contact @a</title>",
                           b"<title>Contact @a</title>"])
        docs.append(head + b"".join(
            rng.choice(_HTML_TOKENS) for _ in range(rng.randrange(0, 30))))
    return docs


def html_corpus():
    """{group: [doc, ...]}: every hand-made t.me document, and one
    fixed-seed fuzz."""
    return {
        "fuzz": html_fuzz_docs(20260304, 1500),
        "table": [d for d, _ in HTML_TABLE_ROWS],
        "rules": html_rule_docs(),
        "edges": [d for _, _, d, _ in html_window_edges()],
        "short": html_short_ranges(),
        "cap": [d for d, _ in html_cap_docs()],
        "packing": html_packing_docs(),
    }


def html_oracle(docs):
    from crawler_amd.engine.htmlvalidator import parse_channel_html

    out = []
    for d in docs:
        r = parse_channel_html(d)
        out.append((r.status, r.reason))
    return out
