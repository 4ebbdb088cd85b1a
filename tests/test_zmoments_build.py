"""Register budget of the phase-matrix moment kernels (csrc/mom_zmom.hip): k_zmom_prt keeps the two previous orders of P, R, T in
registers inside a serial loop over l, and the three instantiations of k_zmom_gemm hold a 2 x 2 block of MFMA accumulators: all
compile for gfx950 without scratch.  No GPU: hipcc cross-compiles, with the Makefile's own command line (make -n) plus
-Rpass-analysis=kernel-resource-usage, into a temporary directory."""
import re
import shlex
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "radiativetransfer.jl_amd" / "csrc"
FIELDS = "Function Name|VGPRs|AGPRs|ScratchSize \\[bytes/lane\\]|Occupancy \\[waves/SIMD\\]|LDS Size \\[bytes/block\\]"


def _resource_usage(tmp_path):
    lines = subprocess.check_output(["make", "-n", "-B", "mom_zmom.o"], cwd=CSRC, text=True).splitlines()
    cmd = shlex.split(next(l for l in lines if "mom_zmom.hip" in l and "-c" in l))
    cmd = [a for a in cmd if a not in ("-MMD", "-MP")]
    cmd[cmd.index("-o") + 1] = str(tmp_path / "mom_zmom.o")
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


def test_moment_kernels_have_no_scratch(tmp_path):
    usage = _resource_usage(tmp_path)
    prt = {k: v for k, v in usage.items() if "k_zmom_prt" in k}
    gemm = {k: v for k, v in usage.items() if "k_zmom_gemm" in k}
    assert len(prt) == 1 and len(gemm) == 3, sorted(usage)   # k_zmom_gemm<n>, n = 1, 3, 4
    for k, v in sorted({**prt, **gemm}.items()):
        print(f"{k}: VGPRs {v['VGPRs']}, AGPRs {v['AGPRs']}, LDS {v['LDS Size [bytes/block]']} B/block, "
              f"scratch {v['ScratchSize [bytes/lane]']} B/lane, occupancy {v['Occupancy [waves/SIMD]']}")
        assert v["ScratchSize [bytes/lane]"] == 0, k
    for k, v in gemm.items():
        assert v["LDS Size [bytes/block]"] == 2 * 16 * 80 * 8, k   # two staged factors of 16 k rows, pitch 80
        assert v["Occupancy [waves/SIMD]"] >= 4, k                  # several workgroups per CU hide the staging's global loads
