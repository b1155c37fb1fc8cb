"""The instruction budget of the shade kernels (scripts/analysis/shade_instruction_budget.py) on the listing the build makes: the `; SECTION` marks of
shade_body.h partition each kernel -- every instruction lies in exactly one section -- and the sections' totals are the kernel's total, class by class.
The table itself (static counts x the trip counts of shade_trips.py, reconciled with the SQ counters) is under profiles/; this guards the parser and the
marks it rests on.  No GPU needed."""
import importlib.util
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
spec = importlib.util.spec_from_file_location("shade_instruction_budget", ROOT / "scripts" / "analysis" / "shade_instruction_budget.py")
budget = importlib.util.module_from_spec(spec)
spec.loader.exec_module(budget)

KERNELS = ["k2_shade", "k2_shade_p", "k2_shade_t", "k2_shade_pt", "k2_shade_pt_w", "k2_shade_csm_pt", "k2_shade_ibl_pt", "k2_shade_band_pt"]
# every mark a kernel may carry (a kernel need not have all of them: the K3 kernels shade their directional lights before the windows)
SECTIONS = {"entry", "entry_ragged", "setup", "lane_pass_0", "lane_pass_1", "window_control", "window_general", "light_general", "light_test_point",
            "light_test_spot", "light_reach", "light_append", "light_next", "pair_pass", "sum_up", "sum_round", "directional", "directional_light",
            "epilogue", "out_of_line"}


@pytest.fixture(scope="module")
def listing():
    assert budget.LISTING.exists(), f"{budget.LISTING} is missing: run __graft_entry__.build()"
    return budget.LISTING.read_text()


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_sections_partition_the_kernel(listing, kernel):
    insns = budget.parse_kernel(listing, kernel)
    body = budget.kernel_lines(listing, kernel)
    # every line of the kernel that is an instruction -- found here without the parser: a tab, a mnemonic, not a directive, a label or a comment --
    # has exactly one entry, in listing order, and the entry names one of the known sections
    plain = [l.split()[0] for l in body if re.match(r"^\s+[a-z]\w*(\s|$)", l) and not l.lstrip().startswith((".", ";"))]
    assert [op for _sec, _cls, op in insns] == plain
    assert len(plain) > 1000
    assert {sec for sec, _cls, _op in insns} <= SECTIONS, {sec for sec, _cls, _op in insns} - SECTIONS
    assert all(cls in budget.CLASSES for _sec, cls, _op in insns)


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_section_totals_are_the_kernels_total(listing, kernel):
    table = budget.section_table(budget.parse_kernel(listing, kernel))
    total = budget.kernel_total(listing, kernel)      # counted without looking at the marks
    for cls in budget.CLASSES:
        assert sum(counts[cls] for counts in table.values()) == total[cls], cls
    assert sum(total.values()) == sum(sum(c.values()) for c in table.values())


def test_the_flagship_kernel_carries_every_section_of_the_table(listing):
    table = budget.section_table(budget.parse_kernel(listing, "k2_shade_pt"))
    rows = budget.budget(budget.parse_kernel(listing, "k2_shade_pt"), budget.parse_trips(budget.DEFAULT_TRIPS_TEXT))
    assert set(table) == SECTIONS
    assert [r[0] for r in rows] == list(table)
    # the hand-written loop: its per-light sections exist once per (kind, list half) and cost the same in each copy
    for sec, copies in budget.COPIES.items():
        if not sec.startswith("light_"):
            continue
        assert sum(table[sec][c] for c in budget.COUNTED) % copies in (0, copies // 2), (sec, table[sec])   # (the second half's copy has one instruction more)
    text = budget.format_table(rows)
    assert "model, per wave" in text and "fixed cost per wave" in text


def test_the_counters_file_is_read():
    c = budget.parse_counters("k2_shade_pt waves 129600\n   SQ_INSTS_VALU   65904456   per wave      508.5\n   SQ_INSTS_VMEM_RD  591210   per wave  4.6\n"
                              "   SQ_INSTS_VMEM_WR   129600   per wave        1.0\n")
    assert c["VALU"] == 508.5 and c["VMEM"] == 5.6 and c["SALU"] == 0.0


def test_the_addressing_rule_on_both_sides_of_4_gb(tmp_path):
    """scripts/shade_addressing_host_check.cpp -- host_rules.h's shade_planes_fit_32_bits against the statement it stands for, worked out in arithmetic that
    cannot wrap -- built with the host sanitizers and run (plain C++: no device, no library)."""
    if not shutil.which("g++"):
        pytest.skip("no host compiler here")
    exe = tmp_path / "shade_addressing_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    str(ROOT / "scripts" / "shade_addressing_host_check.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "shade_addressing_host_check: ok" in run.stdout, run.stdout + run.stderr
