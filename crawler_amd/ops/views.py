"""The kernels' pointer views, read from ``csrc/views.h``: one field table
per view (``BatchView``, ``LinkOut``, ``YtView``, ``TemplateTables`` and
the three feedgen output lists), parsed as text once.

:func:`bind` packs a view's ``void**`` array in the table's order.
``lookup`` maps a field name to a tensor, or None. The drivers resolve a
name (:func:`lookup_in`) in ``batch.meta`` first, then as a batch
attribute, then in the extras dict they pass; a field two sources could
supply is told apart by its name in the table (the batch's ``text_pool``
is the table's ``pool``, passed as an extra)."""
from __future__ import annotations

import ctypes
import os
import re

import torch

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc",
                      "views.h")
DTYPES = {"int": torch.int32, "long": torch.int64,
          "long long": torch.int64, "unsigned long long": torch.int64,
          "unsigned char": torch.uint8, "double": torch.float64}


def parse(text: str) -> dict:
    """{view: [(field, dtype), ...]} of every ``<View>_FIELDS(F)`` list,
    numbered segments spliced in where a list names them."""
    text = re.sub(r"//.*", "", text).replace("\\\n", " ")
    lists = {}
    for name, body in re.findall(r"^#define (\w+)\(F\)(.*)$", text, re.M):
        fields = []
        for ctype, arg in re.findall(r"(\w+)\(F\)|F\(([^()]*)\)", body):
            if ctype:
                fields += lists[ctype]
                continue
            ctype, _, field = arg.rpartition(",")
            elem = re.sub(r"\b(const|__restrict__)\b|\*", "", ctype)
            elem = " ".join(elem.split())
            if elem not in DTYPES or "*" not in ctype:
                raise ValueError(f"{name}: {field.strip()} has the unknown "
                                 f"pointer type '{ctype.strip()}'")
            fields.append((field.strip(), DTYPES[elem]))
        if re.sub(r"\w+\(F\)|F\([^()]*\)", "", body).strip():
            raise ValueError(f"{name}: not a list of F(type, name): {body}")
        lists[name] = fields
    return {k[:-len("_FIELDS")]: v for k, v in lists.items()
            if k.endswith("_FIELDS")}


VIEWS = parse(open(HEADER).read())


def lookup_in(batch, extras=None):
    """The drivers' lookup rule (see the module docstring)."""
    meta = getattr(batch, "meta", {})
    extras = extras or {}

    def lookup(name):
        if name in meta:
            return meta[name]
        if hasattr(batch, name):
            return getattr(batch, name)
        return extras.get(name)
    return lookup


def bind(view: str, lookup, device):
    """The ctypes ``void*`` array of ``view``'s tensors, in table order.
    Raises ValueError, before anything is launched, for a tensor that is
    missing, on another device than ``device``, not contiguous, or of a
    dtype other than the field's C element type."""
    device = torch.device(device)
    fields = VIEWS[view]
    arr = (ctypes.c_void_p * len(fields))()
    for k, (name, dtype) in enumerate(fields):
        t = lookup(name)
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{view}.{name}: no tensor (got {t!r})")
        same = t.device.type == device.type and (
            device.index is None or t.device.index == device.index)
        if not same or not t.is_contiguous() or t.dtype != dtype:
            raise ValueError(
                f"{view}.{name}: expected a contiguous {dtype} tensor on "
                f"{device}, got {t.dtype} on {t.device}"
                f"{'' if t.is_contiguous() else ', not contiguous'}")
        arr[k] = t.data_ptr()
    return arr
