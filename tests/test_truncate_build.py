"""Resource budget of the δ-BGE truncation kernels (csrc/mom_trunc.hip): all four compile for gfx950 without scratch, the Gram
product stages two factors of 16 nodes, and the solve's LDS image -- the 128 x 128 factor at row pitch 129, four right-hand sides,
four solutions under correction, the value solution and the diagonal -- is the 142336 bytes DESIGN states, within the 160 KiB of a CU.  No GPU: hipcc cross-compiles,
with the Makefile's own command line (make -n) plus -Rpass-analysis=kernel-resource-usage, into a temporary directory."""
import re
import shlex
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "radiativetransfer.jl_amd" / "csrc"
FIELDS = "Function Name|VGPRs|AGPRs|ScratchSize \\[bytes/lane\\]|Occupancy \\[waves/SIMD\\]|LDS Size \\[bytes/block\\]"
SOLVE_LDS = (128 * 129 + (2 * 4 + 2) * 128) * 8


def _resource_usage(tmp_path):
    lines = subprocess.check_output(["make", "-n", "-B", "mom_trunc.o"], cwd=CSRC, text=True).splitlines()
    cmd = shlex.split(next(l for l in lines if "mom_trunc.hip" in l and "-c" in l))
    cmd = [a for a in cmd if a not in ("-MMD", "-MP")]
    cmd[cmd.index("-o") + 1] = str(tmp_path / "mom_trunc.o")
    cmd.append("-Rpass-analysis=kernel-resource-usage")
    log = subprocess.run(cmd, cwd=CSRC, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True).stdout
    out, name = {}, None
    for l in log.splitlines():
        m = re.search(rf"remark: +({FIELDS}): (\S+)", l)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = m.group(2)
            out[name] = {}
        elif name is not None:
            out[name][m.group(1)] = int(m.group(2))
    return out


def test_truncation_kernels_fit(tmp_path):
    usage = _resource_usage(tmp_path)
    kernels = {k: next(v for n, v in usage.items() if k in n) for k in ("k_trunc_weights", "k_trunc_gram", "k_trunc_solve", "k_trunc_mark")}
    assert len(usage) == 4, sorted(usage)
    for k, v in kernels.items():
        print(f"{k}: VGPRs {v['VGPRs']}, AGPRs {v['AGPRs']}, LDS {v['LDS Size [bytes/block]']} B/block, "
              f"scratch {v['ScratchSize [bytes/lane]']} B/lane, occupancy {v['Occupancy [waves/SIMD]']}")
        assert v["ScratchSize [bytes/lane]"] == 0, k
    assert kernels["k_trunc_gram"]["LDS Size [bytes/block]"] == 2 * 16 * 80 * 8   # two staged factors of 16 nodes, pitch 80
    assert kernels["k_trunc_gram"]["Occupancy [waves/SIMD]"] >= 4               # several workgroups per CU hide the staging's loads
    assert SOLVE_LDS == 142336 and kernels["k_trunc_solve"]["LDS Size [bytes/block]"] == SOLVE_LDS <= 160 * 1024
    design = (ROOT / "DESIGN.md").read_text()
    assert f"{SOLVE_LDS} B" in design and "k_trunc_solve" in design   # the figure DESIGN states


def test_tables_come_from_the_mie_unit():
    """P and P² are k_mie_tables' (shared through mom_host.hpp): the truncation unit has no table recurrence of its own"""
    text = (CSRC / "mom_trunc.hip").read_text()
    assert "mom_legendre_tables_launch" in text and "mom_legendre_tables_launch" in (CSRC / "mom_host.hpp").read_text()
    assert "__global__" in text and text.count("__launch_bounds__") == 4
