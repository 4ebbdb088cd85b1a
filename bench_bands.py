#!/usr/bin/env python3
"""Band-resolved aerosol optics (k_optics_bands, k_optics_bands_dual in csrc/mom_optics.hip) as a benchmark; prints one JSON line,
`bench_bands.py OUT.json` also writes it (committed as profiles/bands_bench.json).  `--S N` sets the spectral points (default
scene_C3's 29 944), `--repeats R` the timed runs per leg (default 5; the median is reported beside the minimum and the spread).

1. scenes.scene_C3_bands against scenes.scene_C3 at the same S through mom_rt_run: points/s.  K = 4 bases against K = 2 through the
   same layer images; the difference is the cost of the two bases per point whose weight is an exact zero.
2. scene_C3 itself is leg 1's baseline: run this file at the parent commit's scene_C3 (or bench.py) for the comparison across commits.
3. The device assembly at the C3 shape: wall time of mom_scene_set_optics_bands (uploads, k_optics_bands, the ndoubl loop and the
   scene tail; the value kernel has no events of its own) and the HIP-event time of k_optics_bands_dual at P = 3 (mom_timers right
   after mom_scene_set_optics_bands_partials), beside the wall time of the host twins for the same assembly
   (corert.construct_layer_inputs, absorption.optics_partials_host).
4. Host time of corert.z_bases for the banded scene (K = 4: each (m, Greek set) once) and for scene_C3 (K = 2, each pair twice)."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def timed(fn, repeats, warmup=1):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--S", type=int, default=29_944)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import rtamd
    rt, ab = rtamd.corert, rtamd.absorption
    res = {"S": a.S, "repeats": a.repeats}
    models = {"scene_C3": rtamd.scenes.scene_C3(a.S), "scene_C3_bands": rtamd.scenes.scene_C3_bands(a.S)}

    # 4. z_bases on the host
    res["z_bases_host_ms"] = {name: spread(timed(lambda m=m: rt.z_bases(m), 3, warmup=0)) for name, m in models.items()}

    # 1. / 2. the sweep: mom_rt_run of the resident scene, synchronised by the read-back of R_SFI / T_SFI
    sweep = {}
    for name, m in models.items():
        with rt.make_handle(m) as h:
            t0 = time.perf_counter()
            rt.scene_set_device_optics(h, m, upload_tau_abs=True)
            set_ms = (time.perf_counter() - t0) * 1e3

            def run():
                h.rt_run()
                h.sync()
            ms = timed(run, a.repeats, warmup=2)
            dev = h.timers()
            K = int(h._K)
            R, _ = h.get_RT()
        sweep[name] = {"K": K, "rt_run_wall_ms": spread(ms), "points_per_s": a.S / (statistics.median(ms) * 1e-3),
                       "rt_run_device_total_ms": float(dev["total_ms"]), "first_scene_set_wall_ms": set_ms, "finite": bool(np.isfinite(R).all())}
    sweep["bands_over_unbanded_time"] = sweep["scene_C3_bands"]["rt_run_wall_ms"]["median"] / sweep["scene_C3"]["rt_run_wall_ms"]["median"]
    res["sweep"] = sweep

    # 3. the assembly, device and host
    m = models["scene_C3_bands"]
    Nz = m.τ_rayl.shape[1]
    bd = m.bands
    dω̃ = np.array([[x.ω̃ for x in band] for band in bd.aerosol_optics])
    ps = [rt.OpticsPartial(w_gas=np.ones(Nz)), rt.OpticsPartial(dτ_aer=bd.τ_aer.copy()), rt.OpticsPartial(dω̃=dω̃, w_rayl=np.ones(Nz))]
    Zpp, Zmp = rt.z_bases(m)
    with rt.make_handle(m) as h:
        import unittest.mock as mock
        with mock.patch.object(rt, "z_bases", lambda model: (Zpp, Zmp)):   # the bases are leg 4's; here the assembly alone
            h.absorption_set(m.τ_abs)   # the resident τ_abs table goes up once; the timed calls assemble from it
            set_ms = timed(lambda: rt.scene_set_device_optics(h, m, upload_tau_abs=False), a.repeats)
            dual_wall, dual_dev = [], []
            for _ in range(a.repeats + 1):
                t0 = time.perf_counter()
                rt.scene_set_optics_partials(h, m, ps, surf_kind=0)
                dual_wall.append((time.perf_counter() - t0) * 1e3)
                dual_dev.append(float(h.timers()["total_ms"]))
    host_val = timed(lambda: rt.construct_layer_inputs(m), 3, warmup=0)
    host_dual = timed(lambda: ab.optics_partials_host(m, ps), 3, warmup=0)
    res["assembly"] = {"P": len(ps), "Nz": Nz, "K": int(Zpp.shape[1]),
                       "mom_scene_set_optics_bands_wall_ms": spread(set_ms),
                       "mom_scene_set_optics_bands_partials_wall_ms": spread(dual_wall[1:]),
                       "k_optics_bands_dual_hip_event_ms": spread(dual_dev[1:]),
                       "host_twin_construct_layer_inputs_ms": spread(host_val), "host_twin_optics_partials_host_ms": spread(host_dual)}
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
