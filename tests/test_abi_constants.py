"""CPU: the named words of the rasterizer's ABI -- the forward / backward flags, the overflow and tiers words, the return
codes -- carry the same values in include/manus_hip.h, in manus_amd/_lib.py and in the table below, which pins the numbers
themselves (callers outside this tree pass them as plain ints)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WANT = dict(
    MGR_OK=0, MGR_EINVAL=-1, MGR_ENOMEM=-2, MGR_EHIP=-3, MGR_EOVERFLOW=-4, MGR_ECUT=-6, MGR_ETIER=-7, MGR_ESTATE=-8,
    MGR_FWD_CHECK=1, MGR_FWD_NO_BLEND=2, MGR_FWD_BLEND_ONLY=4, MGR_FWD_DEPTH_CUT=8, MGR_FWD_SKIP_BOX_LARGE=16,
    MGR_FWD_SKIP_BOX_MID=32, MGR_FWD_SKIP_SORT_BEHIND=128, MGR_FWD_RANK_LARGE=256, MGR_FWD_IMAGE_KEPT=1024,
    MGR_FWD_REPAIR=2048, MGR_FWD_SPREAD=4096,
    MGR_BWD_CHECK=1, MGR_BWD_OUTPUTS_KEPT=512,
    MGR_OVF_PAIRS=1, MGR_OVF_CUT=2, MGR_OVF_TIER=4, MGR_OVF_FLAGS_MASK=0xFFFF, MGR_OVF_REPAIRED_SHIFT=16,
    MGR_TIERS_BOX_LARGE=1, MGR_TIERS_BOX_MID=2, MGR_TIERS_WIDE_RECT=4, MGR_TIERS_NEAR_SMALL_SHIFT=8,
    MGR_TIERS_NEAR_LARGE_SHIFT=16, MGR_TIERS_NEAR_MASK=0xFF, MGR_TIERS_BEYOND_SMALL_SHIFT=24, MGR_TIERS_BEYOND_SMALL_MASK=0x7F)


def _header_values(path):
    """{name: value} of the `#define MGR_X <int>` lines and the `MGR_X = <int>` enumerators of a header."""
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    found = re.findall(r"^\s*#define\s+(MGR_\w+)\s+(-?(?:0x[0-9A-Fa-f]+|\d+))u?\s*$", text, flags=re.M)
    found += re.findall(r"\b(MGR_\w+)\s*=\s*(-?\d+)\s*[,}\n]", text)
    return {name: int(value, 0) for name, value in found}


def test_abi_words_have_one_value_everywhere():
    from manus_amd import _lib
    hdr = _header_values(os.path.join(ROOT, "include", "manus_hip.h"))
    for name, value in WANT.items():
        assert hdr.get(name) == value, (name, hdr.get(name))
        assert getattr(_lib, name) == value, name
    # every word of these families that the header names is mirrored and pinned: a new flag cannot be added on one side only
    families = ("MGR_E", "MGR_OK", "MGR_FWD_", "MGR_BWD_", "MGR_OVF_", "MGR_TIERS_")
    assert {n for n in hdr if n.startswith(families)} == set(WANT)
    assert {n for n in vars(_lib) if n.startswith(families)} == set(WANT)
    # the forward's flags are independent bits
    fwd = [v for n, v in WANT.items() if n.startswith("MGR_FWD_")]
    assert all(v & (v - 1) == 0 for v in fwd) and len(set(fwd)) == len(fwd) == 11


def test_private_header_leaves_the_overflow_bits_to_the_public_one():
    text = open(os.path.join(ROOT, "manus_amd", "csrc", "mgr_common.h")).read()
    assert not re.search(r"#\s*define\s+MGR_OVF_", text)
    assert not any(n.startswith("MGR_OVF_") for n in _header_values(os.path.join(ROOT, "manus_amd", "csrc", "mgr_common.h")))
    assert re.search(r'#include\s+"\.\./\.\./include/manus_hip\.h"', text)
