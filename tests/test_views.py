"""ops/csrc/views.h, the single table of the kernels' pointer views:
that it parses, that the .hip sources generate their structs from it, and
that ``views.bind`` packs and checks tensors against it. Also the driver
helpers that sit beside it (``_alloc_out``, ``_excl_offsets``). CPU only:
nothing is loaded or launched."""
import os
import re

import numpy as np
import pytest
import torch

from crawler_amd.feed.synth import FeedConfig, SyntheticFeed
from crawler_amd.ops import gpu, views

CSRC = os.path.dirname(views.HEADER)
HEADER_TEXT = open(views.HEADER).read()
# struct -> the source that declares it; the feedgen output lists have no
# struct, their entry points unpack them into locals
STRUCTS = {"BatchView": "parse_encode.hip", "LinkOut": "parse_encode.hip",
           "YtView": "yt_encode.hip", "TemplateTables": "feedgen.hip"}
OUTPUT_LISTS = ["FeedMetaOut", "FeedFillOut", "FeedCommentOut"]


# ---- the header ----

def test_every_list_in_the_header_parses():
    named = set(re.findall(r"^#define (\w+)_FIELDS\(F\)", HEADER_TEXT, re.M))
    assert named == set(STRUCTS) | set(OUTPUT_LISTS)
    assert set(views.VIEWS) == named
    assert {v: len(f) for v, f in views.VIEWS.items()} == {
        "BatchView": 49, "LinkOut": 5, "YtView": 28, "TemplateTables": 19,
        "FeedMetaOut": 18, "FeedFillOut": 9, "FeedCommentOut": 9}


@pytest.mark.parametrize("view", sorted(views.VIEWS))
def test_field_names_are_unique_and_typed(view):
    names = [name for name, _ in views.VIEWS[view]]
    assert len(set(names)) == len(names)
    assert all(dtype in set(views.DTYPES.values())
               for _, dtype in views.VIEWS[view])


def test_every_c_element_type_in_the_header_maps_to_a_dtype():
    text = re.sub(r"//.*", "", HEADER_TEXT)
    ctypes_ = {m.rpartition(",")[0] for m in re.findall(r"\bF\(([^()]*)\)",
                                                        text)}
    elems = {" ".join(re.sub(r"\b(const|__restrict__)\b|\*", "", c).split())
             for c in ctypes_}
    assert elems and elems <= set(views.DTYPES)
    assert views.DTYPES["unsigned long long"] == torch.int64
    assert views.DTYPES["int"] == torch.int32
    assert views.DTYPES["unsigned char"] == torch.uint8
    assert views.DTYPES["double"] == torch.float64


def test_segments_splice_in_order():
    got = views.parse("#define V_FIELDS_0(F) \\\n  F(const int*, a)\n"
                      "#define V_FIELDS_1(F) F(long* __restrict__, b)\n"
                      "#define V_FIELDS(F) \\\n  V_FIELDS_0(F) V_FIELDS_1(F)\n")
    assert got == {"V": [("a", torch.int32), ("b", torch.int64)]}


@pytest.mark.parametrize("body", [
    "F(const float*, x)",        # no dtype for the element type
    "F(const short*, x)",
    "F(int, x)",                 # not a pointer
    "F(const int*, x) int n;",   # something that is no field
])
def test_an_unknown_type_or_a_stray_member_raises(body):
    with pytest.raises(ValueError, match="W_FIELDS"):
        views.parse(f"#define W_FIELDS(F) {body}\n")


# ---- the .hip sources against the header ----

def _struct_body(view):
    text = open(os.path.join(CSRC, STRUCTS[view])).read()
    m = re.search(r"^struct %s \{\n(.*?)^\};" % view, text, re.M | re.S)
    assert m, f"struct {view} not found"
    return re.sub(r"//.*", "", m.group(1)), text


@pytest.mark.parametrize("view", sorted(STRUCTS))
def test_struct_members_are_generated_from_the_table(view):
    body, text = _struct_body(view)
    segments = re.findall(r"^#define (%s_FIELDS_\d+)\(F\)" % view,
                          HEADER_TEXT, re.M) or [view + "_FIELDS"]
    used = re.findall(r"(\w+)\(VIEW_MEMBER\)", body)
    assert used == segments
    assert "*" not in body, "a pointer member is hand-written"
    assert text.count(view + "_FIELDS(VIEW_UNPACK)") == 1


@pytest.mark.parametrize("view", OUTPUT_LISTS)
def test_feedgen_outputs_are_unpacked_from_the_table(view):
    text = open(os.path.join(CSRC, "feedgen.hip")).read()
    assert text.count(view + "_FIELDS(VIEW_LOCAL)") == 1
    assert "out_ptrs[" not in text


def test_ptr_counts_are_the_tables_lengths():
    for src, fn, view in (("parse_encode.hip", "crawl_batch_ptr_count",
                           "BatchView"),
                          ("yt_encode.hip", "crawl_yt_ptr_count", "YtView")):
        text = open(os.path.join(CSRC, src)).read()
        assert ("int %s() { return 0 %s_FIELDS(VIEW_COUNT); }"
                % (fn, view)) in text


# ---- bind ----

def _link_tensors(n=3):
    L = gpu.MAX_LINKS
    return {"name": torch.zeros((n, L, 32), dtype=torch.uint8),
            "name_len": torch.zeros((n, L), dtype=torch.uint8),
            "src": torch.zeros((n, L), dtype=torch.uint8),
            "cnt": torch.zeros(n, dtype=torch.int32),
            "hash": torch.zeros((n, L), dtype=torch.int64)}


@pytest.fixture(scope="module")
def batch_sources():
    """A CPU batch from the standard builder and the extras parse_encode
    adds to it."""
    feed = SyntheticFeed(FeedConfig(seed=7, comment_rate=0.5))
    batch = feed.build_batch(np.arange(3, dtype=np.int64), 4)
    stamp = torch.zeros(20, dtype=torch.uint8)
    extras = dict(gpu._const_tables("cpu"), pool=batch.text_pool,
                  created_str=stamp, capture_str=stamp.clone())
    return batch, extras


def _ptrs(arr):
    return [p or 0 for p in arr]


def test_bind_links_in_table_order():
    t = _link_tensors()
    arr = views.bind("LinkOut", t.get, "cpu")
    order = ["name", "name_len", "src", "cnt", "hash"]
    assert [n for n, _ in views.VIEWS["LinkOut"]] == order
    assert _ptrs(arr) == [t[n].data_ptr() for n in order]


def test_bind_batch_view_in_table_order(batch_sources):
    batch, extras = batch_sources
    lookup = views.lookup_in(batch, extras)
    arr = views.bind("BatchView", lookup, "cpu")
    assert len(arr) == 49
    assert _ptrs(arr) == [lookup(n).data_ptr()
                          for n, _ in views.VIEWS["BatchView"]]
    # the lookup rule: meta, then the batch's attributes, then the extras
    assert lookup("views") is batch.meta["views"]
    assert lookup("chat_id") is batch.chat_id
    assert lookup("pool") is batch.text_pool
    assert lookup("emoji_off") is extras["emoji_off"]
    assert lookup("no_such_field") is None


def _broken(view, sources, field, value):
    if view == "LinkOut":
        t = dict(sources)
        if value is None:
            del t[field]
        else:
            t[field] = value
        return t.get
    batch, extras = sources
    inner = views.lookup_in(batch, extras)
    return lambda name: value if name == field else inner(name)


@pytest.mark.parametrize("view,field", [("LinkOut", "cnt"),
                                        ("BatchView", "com_cnt"),
                                        ("BatchView", "ctname_off")])
def test_bind_rejects_a_bad_tensor(view, field, batch_sources):
    sources = _link_tensors() if view == "LinkOut" else batch_sources
    good = _broken(view, sources, field, torch.zeros(8, dtype=torch.int32))
    views.bind(view, good, "cpu")
    bad = {
        "missing": None,
        "int64 in an int field": torch.zeros(8, dtype=torch.int64),
        "strided": torch.zeros(16, dtype=torch.int32)[::2],
        "meta device": torch.zeros(8, dtype=torch.int32, device="meta"),
    }
    assert not bad["strided"].is_contiguous()
    for what, value in bad.items():
        with pytest.raises(ValueError, match=rf"{view}\.{field}\b") as e:
            views.bind(view, _broken(view, sources, field, value), "cpu")
        if what == "int64 in an int field":
            assert "int64" in str(e.value) and "int32" in str(e.value), what
        if what == "meta device":
            assert "meta" in str(e.value), what
        if what == "strided":
            assert "not contiguous" in str(e.value), what


# ---- the driver helpers ----

def test_alloc_out_typed_guard():
    out, raw = gpu._alloc_out(5, "cpu", None, 2, torch.int32)
    assert out.dtype == torch.int32 and out.numel() == 5
    assert raw.dtype == torch.int32 and raw.numel() == 9
    assert out.data_ptr() == raw[2:].data_ptr()
    poison = torch.tensor(0xA5A5A5A5 - (1 << 32), dtype=torch.int32)
    assert (raw[:2] == poison).all() and (raw[7:] == poison).all()

    out, raw = gpu._alloc_out(5, "cpu", 0x5C, 2, torch.int32)
    assert (raw.view(torch.uint8) == 0x5C).all() and raw.numel() == 9
    out, raw = gpu._alloc_out(3, "cpu", 0x5C, 0, torch.int64)
    assert out.numel() == 3 and (out.view(torch.uint8) == 0x5C).all()
    out, raw = gpu._alloc_out(0, "cpu", None, 2, torch.int64)
    assert out.numel() == 0 and raw.numel() == 4


def test_alloc_out_seams_off_is_a_bare_empty():
    for dtype in (torch.uint8, torch.int32, torch.int64):
        out, raw = gpu._alloc_out(6, "cpu", None, 0, dtype)
        assert raw is None
        assert out.dtype == dtype and out.shape == (6,)
        assert out.is_contiguous() and out.storage_offset() == 0
        assert out.untyped_storage().nbytes() == 6 * out.element_size()
    out, raw = gpu._alloc_out(6, "cpu", None, 0)
    assert out.dtype == torch.uint8 and raw is None


@pytest.mark.parametrize("lengths,offsets,total", [
    ([3, 0, 5], [0, 3, 3], 8),
    ([7], [0], 7),
    ([], [], 0),
])
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_exclusive_offsets(lengths, offsets, total, dtype):
    off, tot = gpu._excl_offsets(torch.tensor(lengths, dtype=dtype))
    assert off.dtype == torch.int64 and off.tolist() == offsets
    assert tot == total and isinstance(tot, int)
    assert off.is_contiguous()


def test_exclusive_offsets_do_not_wrap_at_int32():
    off, tot = gpu._excl_offsets(
        torch.tensor([1 << 30, 1 << 30, 1 << 30], dtype=torch.int32))
    assert off.tolist() == [0, 1 << 30, 1 << 31] and tot == 3 << 30
