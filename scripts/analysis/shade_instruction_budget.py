"""Where the instructions of a k2_shade wave go (CPU): the kernel's gfx950 listing, split at the `; SECTION <name>` marks of shade_body.h, counted per
section and class, and multiplied by the trip counts of shade_trips.py on the C3 frame.

The listing is what the Makefile's flags for shade.o give with `-S --cuda-device-only`: sailor_amd/csrc/shade.s, which the build makes beside the library.  A section is everything between one
mark and the next IN LISTING ORDER (several stretches may carry one name: their counts add up); what the compiler places behind the kernel's last
s_endpgm -- the out-of-line blocks of branches it expects not to be taken -- is the section `out_of_line`.  The split is by position: an instruction the
scheduler moved across a mark is counted on the other side of it, and a section's count is its STATIC size -- a branch inside it that skips a part
makes the dynamic count smaller.  The table says which sections that concerns; the residual against the SQ counters is what all of it adds up to.

Classes, as the SQ counters see them: VALU (v_*), SALU (s_* arithmetic, moves, compares), branch (s_branch, s_cbranch_*), LDS (ds_*), SMEM (s_load_*),
VMEM (global_* / buffer_* / flat_* / scratch_*), and `wait`: s_waitcnt, s_nop, s_barrier, s_endpgm and their kin -- issued, but in none of the counters'
classes (SQ_INSTS_SALU does not count them on this part: the listing's scalar total matches it only without them).

Usage:  python scripts/analysis/shade_instruction_budget.py [--listing FILE.s] [--kernel k2_shade_pt] [--trips FILE | --run-trips] [--counters FILE]
        --trips: the saved output of shade_trips.py; --counters: the output of scripts/pmc_summary.py for the same kernel (the residual's other side)."""
import argparse
import re
import subprocess
import sys
from collections import OrderedDict
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
CSRC = ROOT / "sailor_amd" / "csrc"
CLASSES = ("VALU", "SALU", "branch", "LDS", "SMEM", "VMEM", "wait")
COUNTED = ("VALU", "SALU", "branch", "LDS", "SMEM", "VMEM")   # the classes the SQ_INSTS_* counters add up to
WAIT_OPS = ("s_waitcnt", "s_nop", "s_barrier", "s_endpgm", "s_sleep", "s_sethalt", "s_setprio", "s_code_end", "s_inst_prefetch", "s_clause", "s_ttracedata",
            "s_icache_inv", "s_wakeup", "s_trap", "s_incperflevel", "s_decperflevel")
FIRST_SECTION = "entry"

# shade_trips.py on the C3 frame (rows 10, 40, 67, 77, 100, 125; its output is deterministic): the defaults when no --trips file is given
DEFAULT_TRIPS_TEXT = """
list length                mean    22.31
reach >=1 pixel            mean     5.47
>=1 queued pair            mean     4.26
queued pairs               mean    42.38
max pairs of one pixel     mean     1.95
pair passes (ceil(pairs/64)) mean 1.2798611111111111  lane utilisation
quadrants with list < 8: 0.125  < 16: 0.42916666666666664  > 64: 0.044444444444444446
survivors: box 11.872743055555556  sphere@centre pixel 13.169791666666667  sphere@box centre 12.42
           spot lights per list 5.690277777777778  that reach >= 1 pixel 1.5147569444444444  that pass a cone-vs-sphere test 3.5381944444444446  (wrongly
"""


LISTING = CSRC / "shade.s"   # the Makefile's target: shade.o's flags with -S --cuda-device-only


def compile_listing() -> Path:
    """shade.hip -> the device listing (brought up to date by make; the build makes it along with the library)"""
    subprocess.run(["make", "-s", "-C", str(CSRC), "shade.s"], check=True, capture_output=True, text=True)
    return LISTING


def classify(op: str) -> str:
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "VMEM"
    if op.startswith(("s_load_", "s_buffer_load_", "s_memtime", "s_memrealtime")):
        return "SMEM"
    if op.startswith(("s_cbranch_", "s_branch", "s_setpc", "s_swappc", "s_call")):
        return "branch"
    if op.startswith(WAIT_OPS):
        return "wait"
    if op.startswith("s_"):
        return "SALU"
    raise ValueError(f"an instruction of no known class: {op}")


def kernel_lines(text: str, kernel: str):
    """the lines of `kernel` (its unqualified name) from its label to its .Lfunc_end"""
    lines = text.splitlines()
    start = [i for i, l in enumerate(lines) if re.match(rf"_Z{len(kernel)}{re.escape(kernel)}\w*:", l)]
    if len(start) != 1:
        raise ValueError(f"{kernel}: {len(start)} labels in the listing")
    end = next(i for i in range(start[0], len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start[0] + 1:end]


INSN = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")


def parse_kernel(text: str, kernel: str = "k2_shade_pt"):
    """-> a list of (section, class, mnemonic), one entry per instruction of the kernel, in listing order"""
    body = kernel_lines(text, kernel)
    insns = []
    section = FIRST_SECTION
    for i, l in enumerate(body):
        m = re.search(r";\s*SECTION\s+(\w+)", l)
        if m:
            section = m.group(1)
            continue
        if l.lstrip().startswith((";", ".", "//")) or not l.strip():
            continue
        m = INSN.match(l)
        if not m:
            continue   # a label
        op = m.group(1)
        insns.append((section, classify(op), op))
        if op == "s_endpgm" and section == "epilogue":
            section = "out_of_line"
    return insns


def section_table(insns):
    """-> {section: {class: static count}} in the order the sections first appear"""
    t = OrderedDict()
    for sec, cls, _ in insns:
        t.setdefault(sec, dict.fromkeys(CLASSES, 0))[cls] += 1
    return t


# Sections whose stretches are COPIES of one piece of code, of which an execution runs one: the hand-written light loop exists once per list half (and its
# shared parts once per light kind as well), the sum-up's rounds are unrolled.  Their cost per execution is the static count over the number of copies.
COPIES = {"light_test_point": 2, "light_test_spot": 2, "light_reach": 4, "light_append": 4, "light_next": 4, "sum_round": 4}


def kernel_total(text: str, kernel: str = "k2_shade_pt"):
    """the kernel's instructions counted WITHOUT looking at the marks: every line of its body that is an instruction"""
    n = dict.fromkeys(CLASSES, 0)
    for l in kernel_lines(text, kernel):
        if re.search(r";\s*SECTION\s", l) or l.lstrip().startswith((";", ".", "//")):
            continue
        m = INSN.match(l)
        if m:
            n[classify(m.group(1))] += 1
    return n


def parse_trips(text: str) -> dict:
    def num(pat):
        m = re.search(pat, text)
        if not m:
            raise ValueError(f"shade_trips.py output: no match for {pat!r}")
        return float(m.group(1))
    t = {
        "list": num(r"list length\s+mean\s+([\d.]+)"),
        "reach": num(r"reach >=1 pixel\s+mean\s+([\d.]+)"),
        "with_pairs": num(r">=1 queued pair\s+mean\s+([\d.]+)"),
        "pairs": num(r"queued pairs\s+mean\s+([\d.]+)"),
        "sum_rounds": num(r"max pairs of one pixel\s+mean\s+([\d.]+)"),
        "pair_passes": num(r"pair passes \(ceil\(pairs/64\)\) mean\s+([\d.]+)"),
        "second_half": num(r"> 64:\s+([\d.]+)"),
        "sphere": num(r"sphere@centre pixel\s+([\d.]+)"),
        "spots": num(r"spot lights per list\s+([\d.]+)"),
        "spots_reach": num(r"that reach >= 1 pixel\s+([\d.]+)"),
        "spots_cone": num(r"that pass a cone-vs-sphere test\s+([\d.]+)"),
    }
    # lights entering the per-pixel loop: the sphere's survivors, the spot lights among them cut down to those whose cone meets the sphere
    t["enter"] = t["sphere"] - t["spots"] + t["spots_cone"]
    return t


def section_trips(t: dict) -> "OrderedDict[str, tuple[float, str]]":
    """executions per wave of each section, and what the figure is"""
    s = OrderedDict()
    s["entry"] = (1.0, "every wave")
    s["entry_ragged"] = (0.0, "quadrants that cross the frame's edge: none on C3")
    s["setup"] = (1.0, "every wave")
    s["lane_pass_0"] = (1.0, "every wave with a list")
    s["lane_pass_1"] = (t["second_half"], "lists longer than 64")
    s["window_control"] = (1.0, "one window per wave (a second one is rare)")
    s["light_test_point"] = (t["sphere"] - t["spots"], "point lights entering the loop")
    s["light_test_spot"] = (t["spots_cone"], "spot lights entering the loop")
    s["light_reach"] = (t["reach"], "lights reaching a pixel")
    s["light_append"] = (t["with_pairs"], "lights with pairs")
    s["light_next"] = (t["enter"], "lights entering the loop")
    s["light_general"] = (0.0, "ragged or roughness-0 quadrants, lights of no kind: none on C3")
    s["window_general"] = (0.0, "ragged or roughness-0 quadrants: none on C3")
    s["pair_pass"] = (t["pair_passes"], "pair passes")
    s["sum_up"] = (1.0, "once per window")
    s["sum_round"] = (t["sum_rounds"], "sum-up rounds: the most pairs of one pixel")
    s["directional"] = (1.0, "the test for directional lights")
    s["directional_light"] = (0.0, "no directional light on C3")
    s["epilogue"] = (1.0, "every wave")
    s["out_of_line"] = (0.0, "blocks the compiler expects not to run")
    return s


def budget(insns, trips: dict):
    table = section_table(insns)
    st = section_trips(trips)
    rows = []
    for sec, counts in table.items():
        n, what = st.get(sec, (1.0, "(no trip count: taken once)"))
        copies = COPIES.get(sec, 1)
        if copies > 1:
            what += f"; {copies} copies, one runs"
        rows.append((sec, counts, n / copies, what))
    return rows


def format_table(rows, counters=None, title="") -> str:
    out = []
    if title:
        out.append(title)
    head = f"{'section':16s}" + "".join(f"{c:>7s}" for c in CLASSES) + f"{'static':>8s}{'x trips':>9s}{'per wave':>10s}  trips are"
    out.append(head)
    total = dict.fromkeys(CLASSES, 0.0)
    fixed = 0.0
    for sec, counts, n, what in rows:
        static = sum(counts[c] for c in COUNTED)
        out.append(f"{sec:16s}" + "".join(f"{counts[c]:7d}" for c in CLASSES) + f"{static:8d}{n:9.2f}{static * n:10.1f}  {what}")
        for c in CLASSES:
            total[c] += counts[c] * n
        if sec in ("entry", "setup", "lane_pass_0", "window_control", "sum_up", "directional", "epilogue"):
            fixed += static * n
    model = sum(total[c] for c in COUNTED)
    out.append(f"{'model, per wave':16s}" + "".join(f"{total[c]:7.0f}" for c in CLASSES) + f"{'':8s}{'':9s}{model:10.1f}  (the `wait` class is not in the sum)")
    out.append(f"fixed cost per wave (entry, setup, lane_pass_0, window_control, sum_up, directional, epilogue): {fixed:.0f} static instructions")
    if counters:
        measured = sum(counters[c] for c in COUNTED)
        out.append(f"{'SQ counters':16s}" + "".join(f"{counters.get(c, 0.0):7.1f}" for c in CLASSES[:-1]) + f"{'':7s}{'':8s}{'':9s}{measured:10.1f}")
        out.append(f"residual (model - counters): {model - measured:+.1f} instructions a wave = {100.0 * (model - measured) / measured:+.1f} % of the counted total; by class: " +
                   ", ".join(f"{c} {total[c] - counters[c]:+.1f}" for c in COUNTED))
    return "\n".join(out)


def parse_counters(text: str) -> dict:
    def per_wave(name):
        m = re.search(rf"{name}\s+\d+\s+per wave\s+([\d.]+)", text)
        return float(m.group(1)) if m else 0.0
    return {"VALU": per_wave("SQ_INSTS_VALU"), "SALU": per_wave("SQ_INSTS_SALU"), "branch": per_wave("SQ_INSTS_BRANCH"), "LDS": per_wave("SQ_INSTS_LDS"),
            "SMEM": per_wave("SQ_INSTS_SMEM"), "VMEM": per_wave("SQ_INSTS_VMEM_RD") + per_wave("SQ_INSTS_VMEM_WR")}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--listing", default=None, help="the device listing of shade.hip (default: sailor_amd/csrc/shade.s, brought up to date by make)")
    ap.add_argument("--kernel", default="k2_shade_pt")
    ap.add_argument("--trips", default=None, help="saved output of shade_trips.py (default: the figures recorded in this file)")
    ap.add_argument("--run-trips", action="store_true", help="run shade_trips.py now (needs the oracle library)")
    ap.add_argument("--counters", default=None, help="output of scripts/pmc_summary.py for the kernel")
    ap.add_argument("--title", default="")
    a = ap.parse_args()
    text = Path(a.listing).read_text() if a.listing else compile_listing().read_text()
    if a.run_trips:
        trips_text = subprocess.run([sys.executable, str(Path(__file__).with_name("shade_trips.py"))], check=True, capture_output=True, text=True).stdout
    else:
        trips_text = Path(a.trips).read_text() if a.trips else DEFAULT_TRIPS_TEXT
    counters = parse_counters(Path(a.counters).read_text()) if a.counters else None
    insns = parse_kernel(text, a.kernel)
    print(format_table(budget(insns, parse_trips(trips_text)), counters, a.title or f"{a.kernel}: instructions per section (static) and per wave on C3"))


if __name__ == "__main__":
    main()
