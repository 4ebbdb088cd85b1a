"""Register budget of the kernels the spectral Mie call adds (csrc/mom_mie.hip): k_mie_tables compiles for gfx950 without scratch
-- it keeps the two previous orders of six recurrences in registers, and a spill would put them into memory inside a serial
loop.  The spectral call adds no second kernel set: the wavelength is a grid dimension of the kernels test_mie_dual_build.py counts,
so k_mie_sum and k_mie_greek, which gained it too, are looked at here.  No GPU: hipcc cross-compiles, with the Makefile's own
command line (make -n) plus -Rpass-analysis=kernel-resource-usage, into a temporary directory."""
import test_mie_dual_build as build


def test_table_kernel_has_no_scratch(tmp_path):
    usage = build._resource_usage(tmp_path)
    tables = {k: v for k, v in usage.items() if "k_mie_tables" in k}
    assert len(tables) == 1, sorted(usage)
    # one set of kernels serves the single-wavelength and the spectral entry points
    assert sum("k_mie_amp" in k for k in usage) == 7 and sum("k_mie_ab" in k for k in usage) == 4
    assert sum("k_mie_sum" in k for k in usage) == 1 and sum("k_mie_greek" in k for k in usage) == 1
    for k, v in sorted(usage.items()):
        if not any(n in k for n in ("k_mie_tables", "k_mie_sum", "k_mie_greek")):
            continue
        print(f"{k}: VGPRs {v['VGPRs']}, AGPRs {v['AGPRs']}, scratch {v['ScratchSize [bytes/lane]']} B/lane, "
              f"occupancy {v['Occupancy [waves/SIMD]']}")
        assert v["ScratchSize [bytes/lane]"] == 0, k
        assert v["Occupancy [waves/SIMD]"] >= 4, k
