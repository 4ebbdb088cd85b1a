"""Register budget of the PCW kernels (csrc/mom_pcw.hip): every instantiation -- k_pcw_diag<NW, IDX>, k_pcw_gram<NW, SQ>,
k_pcw_combine<MODE>, k_pcw_sums<NO>, k_wigner_tables -- compiles for gfx950 without scratch.  k_pcw_sums<5> holds 60 accumulators
beside the symbol recursion's state and k_pcw_gram<3, false> twelve accumulator tiles; a spill would put the walk's or the product's
inner loop into memory.  No GPU: hipcc cross-compiles, with the Makefile's own command line (make -n) plus
-Rpass-analysis=kernel-resource-usage, into a temporary directory."""
import re
import shlex
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "radiativetransfer.jl_amd" / "csrc"


def _resource_usage(tmp_path):
    lines = subprocess.check_output(["make", "-n", "-B", "mom_pcw.o"], cwd=CSRC, text=True).splitlines()
    cmd = shlex.split(next(l for l in lines if "mom_pcw.hip" in l and "-c" in l))
    cmd = [a for a in cmd if a not in ("-MMD", "-MP")]
    cmd[cmd.index("-o") + 1] = str(tmp_path / "mom_pcw.o")
    cmd.append("-Rpass-analysis=kernel-resource-usage")
    log = subprocess.run(cmd, cwd=CSRC, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True).stdout
    out, name = {}, None
    for l in log.splitlines():
        m = re.search(r"remark: +(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", l)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = m.group(2)
            out[name] = {}
        elif name is not None:
            out[name][m.group(1)] = int(m.group(2))
    return out


def test_pcw_kernels_have_no_scratch(tmp_path):
    usage = _resource_usage(tmp_path)
    count = lambda stem: sum(stem in k for k in usage)
    # diag: NW = 1..3 with and without the index sums; gram: NW = 1..3 and the square product; combine: value, d/dn_r, d/dn_i;
    # sums: 1..5 output rows
    assert (count("k_pcw_diag"), count("k_pcw_gram"), count("k_pcw_combine"), count("k_pcw_sums"), count("k_wigner_tables")) == (6, 4, 3, 5, 1), \
        sorted(usage)
    assert len(usage) == 19, sorted(usage)
    for k, v in sorted(usage.items()):
        print(f"{k}: VGPRs {v['VGPRs']}, AGPRs {v['AGPRs']}, scratch {v['ScratchSize [bytes/lane]']} B/lane, "
              f"occupancy {v['Occupancy [waves/SIMD]']}")
        assert v["ScratchSize [bytes/lane]"] == 0, k
        assert v["VGPRs"] + v["AGPRs"] <= 512, k
