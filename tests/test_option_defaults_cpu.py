"""_lib.OPTION_DEFAULTS, the table that GSWTRenderer.options restores from, against the initialisers of struct Options in
csrc/gswt_ctx.h, read as text (no library load): every member has an entry with its value, every entry has a member -- but for the retired options, which gswt_set_option accepts and stores nowhere."""
import os
import re

from gswt_renderer_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KEY_OF_MEMBER = {
    "no_prefilter": L.GSWT_OPT_NO_LOD_PREFILTER, "debug_varyings": L.GSWT_OPT_DEBUG_VARYINGS, "timing": L.GSWT_OPT_TIMING,
    "segment": L.GSWT_OPT_SEGMENT, "fixed_pair_cap": L.GSWT_OPT_PAIR_CAP, "defer_swap": L.GSWT_OPT_DEFER_SWAP, "graph": L.GSWT_OPT_GRAPH,
    "strict_vs": L.GSWT_OPT_STRICT_VS, "projection": L.GSWT_OPT_PROJECTION, "antialias": L.GSWT_OPT_ANTIALIAS,
    "no_chunk_cull": L.GSWT_OPT_NO_CHUNK_CULL, "no_merge_reuse": L.GSWT_OPT_NO_MERGE_REUSE, "depth_sort": L.GSWT_OPT_DEPTH_SORT,
}
# accepted, stored nowhere: the table keeps them at 0 so that GSWTRenderer.options(COMPOSITE=..., ITEM_ORDER=...) still works
RETIRED = {L.GSWT_OPT_COMPOSITE: 0, L.GSWT_OPT_ITEM_ORDER: 0}


def _members():
    src = open(os.path.join(ROOT, "gswt_renderer_amd", "csrc", "gswt_ctx.h")).read()
    body = re.search(r"struct Options \{(.*?)\n\};", src, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    found = re.findall(r"\bint\s+(\w+)\s*=\s*(-?\d+)\s*;", body)
    assert len(found) == body.count(";")                      # nothing in the struct but `int name = value;`
    return {name: int(value) for name, value in found}


def test_every_member_of_struct_options_has_its_default_in_the_table():
    members = _members()
    assert len(members) == len(KEY_OF_MEMBER) == 13
    for name, value in members.items():
        assert name in KEY_OF_MEMBER, name
        assert L.OPTION_DEFAULTS[KEY_OF_MEMBER[name]] == value, name


def test_every_table_entry_has_a_member():
    members = _members()
    assert len(set(KEY_OF_MEMBER.values())) == len(KEY_OF_MEMBER)
    assert not set(RETIRED) & set(KEY_OF_MEMBER.values())
    assert sorted(L.OPTION_DEFAULTS) == sorted([KEY_OF_MEMBER[name] for name in members] + list(RETIRED))
    assert all(L.OPTION_DEFAULTS[key] == value for key, value in RETIRED.items())
    assert L.GSWT_OPT_DEPTH_PASSES not in L.OPTION_DEFAULTS and L.GSWT_OPT_DEBUG_FLAGS not in L.OPTION_DEFAULTS
    assert L.GSWT_DEFAULT_SEGMENT == L.OPTION_DEFAULTS[L.GSWT_OPT_SEGMENT] == members["segment"]
