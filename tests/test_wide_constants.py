"""CPU checks of the wide-radius additions to the ABI: the Python constants equal the header's, the ABI version and the
timing families moved together."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "mmx.h")) as f:
        return f.read()


def _define(text, name):
    m = re.search(r"^#define\s+%s\s+(-?\w+)" % name, text, re.M)
    assert m, name
    return int(m.group(1), 0)


def _enum(text, name):
    m = re.search(r"\b%s\s*=\s*(-?\w+)" % name, text)
    assert m, name
    return int(m.group(1), 0)


def test_native_constants_equal_the_headers():
    from magellanmapper_amd import _native as nat
    h = _header()
    assert nat.MMX_ABI_VERSION == _define(h, "MMX_ABI_VERSION") == 21
    assert nat.MMX_MAX_RADIUS_WIDE == _define(h, "MMX_MAX_RADIUS_WIDE") == 64
    assert nat.MMX_MAX_RADIUS_FAST == _define(h, "MMX_MAX_RADIUS_FAST") == 24
    assert nat.MMX_ZX_WIDE == _enum(h, "MMX_ZX_WIDE") == 8
    for name in ("MMX_ZX_AUTO", "MMX_ZX_SEPARATE", "MMX_ZX_PACKED", "MMX_ZX_TILED", "MMX_ZX_TILED_Q16"):
        assert getattr(nat, name) == _enum(h, name), name
    assert nat.MMX_MASK_ROWS == _define(h, "MMX_MASK_ROWS") and nat.MMX_MASK_QUADS == _define(h, "MMX_MASK_QUADS")


def test_timing_families_count_fourteen_and_end_with_the_wide_passes():
    from magellanmapper_amd import _native as nat
    h = _header()
    assert len(nat.KERNEL_KINDS) == _define(h, "MMX_K_COUNT") == 14
    assert nat.KERNEL_KINDS[13] == "widepass" and len(set(nat.KERNEL_KINDS)) == 14
    with open(os.path.join(ROOT, "magellanmapper_amd", "csrc", "mmx_common.h")) as f:
        kinds = re.search(r"enum mmx_kernel_kind \{(.*?)\}", f.read(), re.S).group(1)
    names = [k.strip() for k in kinds.replace("= 0", "").split(",")]
    assert names[13] == "MMX_K_WIDE" and names[14] == "MMX_K_END"


def test_built_library_reports_the_new_abi():
    from magellanmapper_amd import _native as nat
    assert nat.lib().mmx_abi_version() == 21


def test_blob_log_reports_rounds_and_layout_beside_the_path():
    from magellanmapper_amd import blob_log as bl
    assert hasattr(bl, "LAST_ZX_PATH") and hasattr(bl, "LAST_PASS_ROUNDS") and hasattr(bl, "LAST_MASK_LAYOUT")
