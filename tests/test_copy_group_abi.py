"""The host validation of hdp_copy_group and of the other grouped stream entries (the merges, the shadow
cast): all of it runs before any launch, so it is testable without a GPU."""
import os

import pytest


def _lib():
    from hdpissa_amd._lib import LIB_PATH, lib
    if not os.path.exists(LIB_PATH):
        pytest.skip("libhdpissa.so not built (run __graft_entry__.build())")
    return lib()


def test_empty_list_is_ok():
    L = _lib()
    assert L.hdp_copy_group(0, None, None) == 0


def test_negative_bytes_is_einval():
    from hdpissa_amd._lib import CopyItem
    L = _lib()
    items = (CopyItem * 2)()
    items[0].dst, items[0].src, items[0].bytes = None, None, 0
    items[1].dst, items[1].src, items[1].bytes = 4096, 8192, -1
    assert L.hdp_copy_group(2, items, None) == 1
    assert b"bytes < 0" in L.hdp_last_error()


@pytest.mark.parametrize("null", ["dst", "src"])
def test_null_pointer_with_bytes_is_einval(null):
    from hdpissa_amd._lib import CopyItem
    L = _lib()
    items = (CopyItem * 1)()
    items[0].dst = None if null == "dst" else 4096
    items[0].src = None if null == "src" else 4096
    items[0].bytes = 16
    assert L.hdp_copy_group(1, items, None) == 1
    assert b"null pointer" in L.hdp_last_error()


def test_null_item_list_is_einval():
    L = _lib()
    assert L.hdp_copy_group(1, None, None) == 1
    assert b"bad item list" in L.hdp_last_error()


# ---- the same for every grouped stream entry: one validation (csrc/hdp_stream_plan.h: stream_check), all of
# ---- it before the first launch.  (name, item class, field names dst / src / count, trailing arguments)
ENTRIES = {
    "merge_f32": ("hdp_merge_group", "MergeItem", ("W", "dW", "n"), (0,)),
    "merge_bf16": ("hdp_merge_group", "MergeItem", ("W", "dW", "n"), (1,)),
    "merge_bf16dw": ("hdp_merge_group_bf16dw", "MergeItem", ("W", "dW", "n"), ()),
    "merge_sr": ("hdp_merge_group_sr", "MergeSrItem", ("W", "dW", "n"), (1234,)),
    "copy": ("hdp_copy_group", "CopyItem", ("dst", "src", "bytes"), ()),
    "shadow": ("hdp_shadow_group", "ShadowItem", ("dst", "src", "n"), ()),
}
HDP_EINVAL = 1


def _entry(key):
    from hdpissa_amd import _lib as M
    name, cls, fields, tail = ENTRIES[key]
    L = _lib()
    fn = getattr(L, name)

    def call(n, items):
        return fn(n, items, *tail, None)

    def make(rows):
        arr = (getattr(M, cls) * len(rows))()
        for it, (dst, src, cnt) in zip(arr, rows):
            setattr(it, fields[0], dst)
            setattr(it, fields[1], src)
            setattr(it, fields[2], cnt)
        return arr
    return L, name.encode(), call, make


@pytest.mark.parametrize("key", list(ENTRIES))
def test_group_empty_list_is_ok(key):
    L, name, call, make = _entry(key)
    assert call(0, None) == 0
    assert call(2, make([(None, None, 0), (None, None, 0)])) == 0  # empty items need no pointers


@pytest.mark.parametrize("key", list(ENTRIES))
def test_group_bad_list_is_einval(key):
    L, name, call, make = _entry(key)
    assert call(1, None) == HDP_EINVAL
    assert name + b": bad item list" in L.hdp_last_error()
    assert call(-1, make([(4096, 8192, 16)])) == HDP_EINVAL
    assert b"bad item list" in L.hdp_last_error()


@pytest.mark.parametrize("null", ["dst", "src"])
@pytest.mark.parametrize("key", list(ENTRIES))
def test_group_null_pointer_is_einval(key, null):
    L, name, call, make = _entry(key)
    row = (None if null == "dst" else 4096, None if null == "src" else 8192, 16)
    assert call(1, make([row])) == HDP_EINVAL
    err = L.hdp_last_error()
    assert name in err and b"item 0" in err and b"null pointer" in err


@pytest.mark.parametrize("key", list(ENTRIES))
def test_group_negative_count_is_einval(key):
    L, name, call, make = _entry(key)
    assert call(1, make([(4096, 8192, -1)])) == HDP_EINVAL
    err = L.hdp_last_error()
    assert b"item 0" in err and (b"bytes < 0" if key == "copy" else b"n < 0") in err


@pytest.mark.parametrize("bad", ["negative", "null"])
@pytest.mark.parametrize("key", list(ENTRIES))
def test_group_bad_second_item_launches_nothing(key, bad):
    """A valid-looking first item must not be merged, copied or cast before the second one is refused: the
    call returns HDP_EINVAL naming item 1.  (An attempt to launch item 0 would come back as a HIP error,
    status 2, on a machine without a GPU, and overwrite W in place on one with.)"""
    L, name, call, make = _entry(key)
    second = (4096 + 65536, 8192 + 65536, -1) if bad == "negative" else (None, 8192 + 65536, 64)
    assert call(2, make([(4096, 8192, 64), second])) == HDP_EINVAL
    err = L.hdp_last_error()
    assert name in err and b"item 1" in err
    assert (b"null pointer" if bad == "null" else (b"bytes < 0" if key == "copy" else b"n < 0")) in err


def test_merge_one_item_entry_validates_like_the_group():
    L = _lib()
    assert L.hdp_merge(None, 0, None, 0, None) == 0
    assert L.hdp_merge(4096, 0, 8192, -1, None) == HDP_EINVAL and b"hdp_merge: " in L.hdp_last_error() \
        and b"n < 0" in L.hdp_last_error()
    assert L.hdp_merge(None, 1, 8192, 8, None) == HDP_EINVAL and b"null pointer" in L.hdp_last_error()
    assert L.hdp_merge(4096, 7, 8192, 8, None) == HDP_EINVAL and b"bad dtype" in L.hdp_last_error()
