"""The two ends of the band kernel's workgroup chain that tile-uniform bookkeeping can lengthen
(tools/isa_budget.py --entry), read from the gfx950 assembly of sem_amd/csrc/apply_band.hip: no GPU.

A workgroup's longest single latency is its first staging load, so what it executes before that load is paid in
full; behind the last barrier an ordinary tile of the CD form needs its LDS reads, a few fp64 operations and its
stores, and every other instruction there is paid by every tile.  The tile map therefore
divides by a host-computed reciprocal (no v_rcp in front of barrier 1), and the tile-uniform decisions of the epilogue
are made before barrier 1.  Both --entry numbers must stay strictly below those of the commit before that change.

One compile per session: the assembly tests/test_band_chain_isa.py made in this session is reused when it is there.
"""
import glob
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tools/isa_budget.py --entry of this file's tool run on the sources of commit d6bf4df (the parent of the change):
# (P, CM) -> (index of the first load through the x buffer resource, instructions last barrier .. last buffer_store)
PARENT = {
    (4, 0): (101, 153), (4, 1): (119, 153),
    (8, 0): (104, 219), (8, 1): (122, 223),
    (12, 0): (104, 388), (12, 1): (125, 389),
    (16, 0): (106, 464), (16, 1): (131, 465),
}


def _tool():
    spec = importlib.util.spec_from_file_location("isa_budget", os.path.join(ROOT, "tools", "isa_budget.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="session")
def band_entry_asm(tmp_path_factory):
    tool = _tool()
    if tool.hipcc() is None:
        pytest.skip("hipcc not found")
    made = glob.glob(os.path.join(str(tmp_path_factory.getbasetemp()), "isa*", "apply_band.s"))
    asm = made[0] if made else tool.compile("apply_band.hip", str(tmp_path_factory.mktemp("isa_entry") / "apply_band.s"))
    return tool, open(asm).read().split("\n")


@pytest.mark.parametrize("cm", [0, 1])
@pytest.mark.parametrize("P", [4, 8, 12, 16])
def test_entry_and_tail_are_shorter_than_the_parents(band_entry_asm, P, cm):
    tool, lines = band_entry_asm
    name, body = tool.kernel_body(lines, "^" + re.escape(tool.mangle(P, False, cm, True)) + "$")
    e = tool.entry(body)
    print(tool.entry_text(name, body))
    assert e["rcp_before_barrier"] == [], tool.entry_text(name, body)   # no runtime division in the tile map
    # the fallback prologue of the preloaded arguments waits once; nothing else may wait in front of the first load
    assert len(e["waits_before_load"]) <= 1, tool.entry_text(name, body)
    first, tail = PARENT[P, cm]
    assert e["first_x_load"] < first, tool.entry_text(name, body)
    assert e["tail"] < tail, tool.entry_text(name, body)


def test_entry_report_sees_what_it_looks_for():
    """The parser on a hand-written body: the first buffer load (not the global load before it), the tail up to the
    last store without its labels, and a reciprocal in front of the first barrier."""
    tool = _tool()
    body = ["global_load_dwordx2 v[0:1], v2, s[0:1]", "v_rcp_iflag_f32_e32 v3, v3",
            "buffer_load_dwordx2 v[4:5], v2, s[4:7], 0 offen", "s_barrier", "v_rcp_f64_e32 v[0:1], v[0:1]", "s_barrier",
            "ds_read_b64 v[0:1], v2", ".LBB0_1:", "buffer_store_dwordx2 v[0:1], v2, s[8:11], 0 offen",
            "buffer_store_dwordx2 v[0:1], v3, s[8:11], 0 offen", "s_endpgm"]
    e = tool.entry(body)
    assert e["first_x_load"] == 2
    assert e["tail"] == 3
    assert [i for i, _ in e["rcp_before_barrier"]] == [1]
    assert e["waits_before_load"] == []
