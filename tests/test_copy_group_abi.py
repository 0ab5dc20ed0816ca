"""hdp_copy_group's host validation: it runs before any launch, so it is testable without a GPU."""
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
