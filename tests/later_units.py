"""What tests/test_gpu_later_units.py shares with its CPU test: the spectral gather of a prepared scene, the same gather on the
model, and the grid bounds of the persistent launches as the sources state them."""
import dataclasses
import re
from pathlib import Path

import numpy as np

CSRC = Path(__file__).resolve().parent.parent / "radiativetransfer.jl_amd" / "csrc"


def take(sc, idx):
    """SceneInputs.spectral_slice for an index array: the points idx[0], idx[1], ... of the spectral axis, in that order.  ndoubl and
    iface stay the global ones (maxima over the whole axis), the bases and the surface matrices do not depend on the point."""
    idx = np.asarray(idx, dtype=np.int64)
    S, Nz, K = sc.S, sc.Nz, sc.K
    g = lambda a, shape: np.ascontiguousarray(np.take(a.reshape(shape), idx, axis=1)).reshape(-1)
    return dataclasses.replace(
        sc, S=int(idx.size), tau=g(sc.tau, (Nz, S)), varpi=g(sc.varpi, (Nz, S)), zw=g(sc.zw, (Nz, S, K)),
        tau_sum=g(sc.tau_sum, (Nz + 1, S)),
        albedo_spec=None if sc.albedo_spec is None else np.ascontiguousarray(np.asarray(sc.albedo_spec)[idx]))


def take_model(m, idx):
    """The model whose prepared scene is take(prepare_scene(m), idx): the gather on the inputs that carry a spectral axis (the
    aerosol columns have none).  For surfaces without a spectral dependence."""
    idx = np.asarray(idx, dtype=np.int64)
    return dataclasses.replace(m, τ_rayl=np.ascontiguousarray(m.τ_rayl[idx]), τ_abs=np.ascontiguousarray(m.τ_abs[idx]))


def source_ints(name, pattern):
    """The integers `pattern` (a regular expression with one group per integer) finds in csrc/<name>; exactly one match"""
    found = re.findall(pattern, (CSRC / name).read_text())
    assert len(found) == 1, (name, pattern, found)
    return tuple(int(x) for x in (found[0] if isinstance(found[0], tuple) else (found[0],)))


def grid_constants():
    """Workgroups per CU of the persistent layer images, the workgroup count of the generic mode and of the batched operators, and
    the point count from which the LDS-resident general kernels take one workgroup per point (looping over the moments)."""
    per_cu = r"static int image_per_cu\(\) \{ return (\d+); \}"
    strip4, strip8 = source_ints("momcore_strip.hip", r"static int image_per_cu\(\) \{ return kWaves == 4 \? (\d+) : (\d+); \}")
    rule = source_ints("mom_scene.hip", r"lds \? \(int\)\(\(a\.S >= (\d+)\) \? a\.S : units\)")[0]
    rule4 = source_ints("mom_scene.hip", r"mom4_launch_layer\(&a, a\.iface, true, \(int\)\(\(a\.S >= (\d+)\) \? a\.S : units\)")[0]
    rule32 = source_ints("momcore_f32.hip", r"lds \? \(int\)\(\(S >= (\d+)\) \? S : S \* M\)")[0]
    assert rule == rule4 == rule32, (rule, rule4, rule32)
    return dict(strip4=strip4, strip8=strip8,
                lean=source_ints("momcore_strip.hip", r"static int lean_image_per_cu\(\) \{ return (\d+); \}")[0],
                lean6=source_ints("momcore_lean6.hip", per_cu)[0], strip2=source_ints("momcore_strip2.hip", per_cu)[0],
                G=source_ints("momcore.hip", r"h->G = (\d+);")[0],
                ops=source_ints("mom_ops.hpp", r"const int grid = lds \? batch : std::min\(batch, (\d+)\);")[0],
                point_rule=rule)


def points_for(bound, moments):
    """The smallest S whose units (S x moments of the launch) give every workgroup of a grid of `bound` two whole rounds and a partial
    third: units >= 2 bound + bound // 2 + 1."""
    return -(-(2 * bound + bound // 2 + 1) // moments)
