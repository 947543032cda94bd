"""the sample chain's option, selection bit and format bit exist in include/fmgpu.h and in capi.py with the stated values and defaults; the ABI version stays 6 (no GPU)"""
import os
import re

from fmindex_collection_amd import capi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fmgpu.h")


def test_option_selection_bit_and_format_bit():
    text = open(HEADER).read()
    assert re.search(r"#define\s+FMGPU_ABI_VERSION\s+6\b", text)
    assert re.search(r"FMGPU_OPT_SAMPLE_CHAIN\s*=\s*12\b", text) and re.search(r"FMGPU_OPT_COUNT_\s*=\s*13\b", text)
    assert capi.OPTIONS["sample_chain"] == 12 and capi.OPTION_DEFAULTS["sample_chain"] == 1
    assert set(capi.OPTIONS) == set(capi.OPTION_DEFAULTS) and sorted(capi.OPTIONS.values()) == list(range(13))
    assert re.search(r"#define\s+FMGPU_SEL_NO_SAMPLE_CHAIN\s+\(1 << 28\)", text) and capi.SEL_NO_SAMPLE_CHAIN == 1 << 28
    sel_all = re.search(r"#define FMGPU_SEL_ALL \((.*?)\)\n", text, re.S).group(1)
    assert "FMGPU_SEL_NO_SAMPLE_CHAIN" in sel_all
    assert re.search(r"#define\s+FMGPU_FMT_CHAIN\s+\(1u << 14\)", text) and capi.FMT_CHAIN == 1 << 14
