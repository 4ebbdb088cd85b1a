"""Register budget of the Mie kernels (csrc/mom_mie.hip): every instantiation of k_mie_ab and k_mie_amp, value and Dual, compiles
for gfx950 without scratch.  The Dual amplitude kernel holds eight accumulator tiles and up to five bulk rows in registers; a spill
would put the epilogue's traffic into memory.  No GPU: hipcc cross-compiles, with the Makefile's own command line (make -n) plus
-Rpass-analysis=kernel-resource-usage, into a temporary directory."""
import re
import shlex
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "radiativetransfer.jl_amd" / "csrc"


def _resource_usage(tmp_path):
    lines = subprocess.check_output(["make", "-n", "-B", "mom_mie.o"], cwd=CSRC, text=True).splitlines()
    cmd = shlex.split(next(l for l in lines if "mom_mie.hip" in l and "-c" in l))
    cmd = [a for a in cmd if a not in ("-MMD", "-MP")]
    cmd[cmd.index("-o") + 1] = str(tmp_path / "mom_mie.o")
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


def test_mie_kernels_have_no_scratch(tmp_path):
    usage = _resource_usage(tmp_path)
    amp = {k: v for k, v in usage.items() if "k_mie_amp" in k}
    ab = {k: v for k, v in usage.items() if "k_mie_ab" in k}
    # k_mie_amp<NW, DUAL>: NW = 1..4 value, 1..3 Dual; k_mie_ab<SCALE, DUAL>: all four
    assert len(amp) == 7 and len(ab) == 4, sorted(usage)
    assert sum("Lb1EEE" in k for k in amp) == 3 and sum("Lb1EEE" in k for k in ab) == 2
    for k, v in sorted({**amp, **ab}.items()):
        print(f"{k}: VGPRs {v['VGPRs']}, AGPRs {v['AGPRs']}, scratch {v['ScratchSize [bytes/lane]']} B/lane, "
              f"occupancy {v['Occupancy [waves/SIMD]']}")
        assert v["ScratchSize [bytes/lane]"] == 0, k
        assert v["VGPRs"] + v["AGPRs"] <= 512, k
