"""Ownership in the C boundary is structural: device and page-locked memory the library allocates for itself lives in the owning
buffers of badslam_amd/csrc/capi_buffers.h, so a new member of the context cannot be forgotten in bahip_context_destroy.  Read from the
sources: no free in the destructor, no raw allocation into the context, no free outside the owning type and the two entry points
that give back memory the CALLER owns."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "badslam_amd", "csrc")
UNITS = sorted(glob.glob(os.path.join(CSRC, "capi*.hip"))) + [os.path.join(CSRC, "capi_internal.h")]
FREE = re.compile(r"\bhip(?:Host)?Free\s*\(")


def _read(path):
    with open(path) as f:
        return f.read()


def _body(text, signature):
    """The braces' contents of the function whose definition starts with `signature`."""
    start = text.index(signature)
    depth, i = 0, text.index("{", start)
    for j in range(i, len(text)):
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return text[i + 1:j]
    raise AssertionError(f"unbalanced braces after {signature}")


def test_the_units_are_there():
    assert len(UNITS) >= 10 and all(os.path.exists(u) for u in UNITS)


def test_context_destruction_frees_nothing_by_hand():
    body = _body(_read(os.path.join(CSRC, "capi.hip")), "void bahip_context_destroy(bahip_context* ctx) {")
    assert "delete ctx" in body
    assert not FREE.search(body), "bahip_context_destroy frees by hand: make the buffer an owning member of the context"


def test_nothing_is_allocated_into_the_context_by_hand():
    for unit in UNITS:
        assert not re.search(r"\bhip(?:Host)?Malloc\s*\(\s*&\s*ctx\s*->", _read(unit)), unit


def test_only_the_owning_type_and_the_callers_entry_points_free():
    allowed = {"capi.hip": ("int bahip_free(void* ptr) {", "int bahip_host_free(void* ptr) {")}
    for unit in UNITS:
        text = _read(unit)
        for signature in allowed.get(os.path.basename(unit), ()):
            body = _body(text, signature)
            assert FREE.search(body), signature
            text = text.replace(body, "")
        assert not FREE.search(text), f"{os.path.basename(unit)} frees device or page-locked memory by hand"
    owning = _read(os.path.join(CSRC, "capi_buffers.h"))
    assert len(FREE.findall(owning)) == 2, "capi_buffers.h: one hipFree and one hipHostFree, in Buffer::release"
    assert FREE.search(_body(owning, "void release() {"))
