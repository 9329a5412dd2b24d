"""What the compiler leaves on the band kernel's dependent chain (tools/isa_budget.py --chain), read from the gfx950
assembly of sem_amd/csrc/apply_band.hip: one device-only compile per session, no GPU.

Between its two barriers a wave contracts the staged window; the u, v loads issued before barrier 1 are meant to
land meanwhile, and every kernel argument is meant to be in SGPRs by then.  A wait for global loads in a role path,
or a scalar load behind barrier 1, puts a memory round trip on every workgroup's chain."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("isa_budget", os.path.join(ROOT, "tools", "isa_budget.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="session")
def band_asm(tmp_path_factory):
    tool = _tool()
    if tool.hipcc() is None:
        pytest.skip("hipcc not found")
    def tree():
        return {os.path.join(d, f) for d, _, fs in os.walk(os.path.join(ROOT, "sem_amd")) for f in fs
                if "__pycache__" not in d}

    before = tree()
    asm = tool.compile("apply_band.hip", str(tmp_path_factory.mktemp("isa") / "apply_band.s"))
    assert tree() == before, "the tool wrote inside the source tree"
    return tool, open(asm).read().split("\n")


@pytest.mark.parametrize("cm", [0, 1])
@pytest.mark.parametrize("P", [4, 8, 12, 16])
def test_no_load_wait_on_the_chain(band_asm, P, cm):
    tool, lines = band_asm
    name, body = tool.kernel_body(lines, "^" + re.escape(tool.mangle(P, False, cm, True)) + "$")
    c = tool.chain(body)
    assert len(c["barriers"]) == 2, c["barriers"]
    assert c["role_vmcnt_waits"] == [], tool.chain_text(name, body)
    assert c["late_scalar_loads"] == [], tool.chain_text(name, body)
    # the epilogue reads all of a thread's X / Y results in one batch: its first LDS wait follows at least the
    # 4 NE result reads (NE = nodes per thread)
    TXE, TYE, NS = tool.band_shape(P)
    lw = 64 * ((TYE * P + 63) // 64)
    waves = TXE * NS * (lw // 64) + NS * ((TXE * P * TYE + 63) // 64)
    ne = -(-TXE * P * lw // (64 * waves))
    assert c["epilogue_lds_waits"][0][2] >= 4 * ne, tool.chain_text(name, body)


def test_chain_report_sees_what_it_looks_for():
    """The parser on a hand-written body: a vmcnt wait between the barriers, a scalar load behind the first one and
    two epilogue wait points are all reported."""
    tool = _tool()
    body = ["buffer_load_dwordx2 v[0:1], v2, s[0:3], 0 offen", "s_waitcnt vmcnt(0)", "s_barrier",
            "s_waitcnt vmcnt(0) lgkmcnt(1)", "s_load_dword s4, s[0:1], 0x80", "s_barrier",
            "ds_read_b64 v[0:1], v2", "s_waitcnt lgkmcnt(0)", "s_waitcnt lgkmcnt(0)", "ds_read2_b64 v[0:3], v2",
            "s_waitcnt vmcnt(1) lgkmcnt(0)"]
    c = tool.chain(body)
    assert [i for i, _ in c["role_vmcnt_waits"]] == [3]
    assert [i for i, _ in c["late_scalar_loads"]] == [4]
    assert [(i, n) for i, _, n in c["epilogue_lds_waits"]] == [(7, 1), (10, 1)]
