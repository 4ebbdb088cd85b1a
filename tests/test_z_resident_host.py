"""The host side of scenes from Greek coefficients (params.z_resident): what needs no GPU -- prepare_scene builds no Z and carries the
Greek sets, spectral_slice keeps them, partials in two forms are refused, and the three descriptions of the new entry points (the
header, _lib.SIGNATURES, integration/MomCore.jl) agree."""
import dataclasses
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
NEW = ("mom_scene_stage_greeks", "mom_scene_stage_greek_partials", "mom_scene_get_bases")


def no_matrices(rtamd, monkeypatch):
    def boom(*a, **kw):
        raise AssertionError("a Z matrix was formed on the z_resident route")
    monkeypatch.setattr(rtamd.corert, "compute_Z_moments_batch", boom)
    monkeypatch.setattr(rtamd.corert, "compute_Z_moments", boom)


def test_prepare_scene_builds_no_z(rtamd, monkeypatch):
    rt = rtamd.corert
    m = rtamd.scenes.make_scene(3, 5, 3, 8, seed=4, z_resident=True)
    assert m.params.z_resident and not rtamd.scenes.make_scene(3, 5, 3, 8, seed=4).params.z_resident
    no_matrices(rtamd, monkeypatch)
    sc = rt.prepare_scene(m)
    assert sc.Zpp is None and sc.Zmp is None
    assert len(sc.greeks) == sc.K == 1 + len(m.aerosol_optics)
    assert sc.greeks[0] is m.greek_rayleigh and sc.greeks[1] is m.aerosol_optics[0].greek_coefs
    with pytest.raises(AssertionError):
        rt.prepare_scene(dataclasses.replace(m, params=dataclasses.replace(m.params, z_resident=False)))


def test_spectral_slice_keeps_the_greek_sets(rtamd):
    rt = rtamd.corert
    sc = rt.prepare_scene(rtamd.scenes.make_scene(1, 3, 3, 8, seed=4, z_resident=True))
    part = sc.spectral_slice(2, 7)
    assert part.S == 5 and part.Zpp is None and part.Zmp is None and part.greeks is sc.greeks
    host = rt.prepare_scene(rtamd.scenes.make_scene(1, 3, 3, 8, seed=4))
    assert host.greeks is None and host.spectral_slice(2, 7).greeks is None and host.spectral_slice(2, 7).Zpp is host.Zpp


class Recorder:
    """stands in for a handle: records the staging call"""
    def __init__(self):
        self.calls = []

    def scene_stage_greek_partials(self, P, pairs):
        self.calls.append((P, [kp for kp, _ in pairs]))


@pytest.mark.parametrize("kind", ["ScenePartial", "OpticsPartial"])
def test_partials_in_two_forms_are_refused(rtamd, kind):
    rt = rtamd.corert
    Partial = getattr(rt, kind)
    g = rt.get_greek_rayleigh(0.1)
    h = Recorder()
    with pytest.raises(ValueError, match="d_greeks"):
        rt.stage_greek_partials(h, [Partial(d_greeks=[(1, g)]), Partial(dZpp=np.zeros((1, 2, 3, 3)), dZmp=np.zeros((1, 2, 3, 3)))])
    assert not h.calls
    assert rt.stage_greek_partials(h, [Partial(), Partial(dZpp=np.zeros((1, 2, 3, 3)))]) is False and not h.calls
    assert rt.stage_greek_partials(h, [Partial(d_greeks=[(1, g)]), Partial(), Partial(d_greeks=[(2, g), (0, g)])]) is True
    assert h.calls == [(3, [(1, 0), (2, 2), (0, 2)])]


def test_resident_aerosol_partials_form_no_matrix(rtamd, monkeypatch):
    rt = rtamd.corert
    m = rtamd.scenes.make_scene(3, 5, 3, 8, seed=4, z_resident=True)
    d = rt.AerosolOptics(rtamd.scenes.hg_like_greek(0.6, len(m.aerosol_optics[0].greek_coefs.β)), 0.1, 0.05)
    no_matrices(rtamd, monkeypatch)
    (p,) = rtamd.scattering.aerosol_optics_partials(m, [(0, d, None, None)], resident=True)
    assert p.dZpp is None and p.dZmp is None and len(p.d_greeks) == 1
    assert p.d_greeks[0][0] == 1 and p.d_greeks[0][1] is d.greek_coefs
    assert p.dω̃[0] == 0.1 and p.dfᵗ[0] == 0.05


def test_header_lib_and_julia_agree(rtamd):
    header = (ROOT / "include" / "momcore.h").read_text()
    julia = (ROOT / "integration" / "MomCore.jl").read_text()
    for name in NEW:
        proto = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M | re.S)
        assert proto, name
        nargs = len(proto.group(1).split(","))
        restype, argtypes = rtamd._lib.SIGNATURES[name]
        assert len(argtypes) == nargs, name
        call = re.search(r"ccall\(\(:" + name + r", libmomcore\), Cint, \(([^)]*)\)", julia)
        assert call and len([t for t in call.group(1).split(",") if t.strip()]) == nargs, name
        assert hasattr(rtamd.load(), name)
    assert subprocess.run([sys.executable, str(ROOT / "tools" / "gen_julia_bindings.py"), "--check"]).returncode == 0
    rt_jl = (ROOT / "integration" / "MomCoreRT.jl").read_text()
    assert "mom_scene_stage_greeks!" in rt_jl and "z_resident" in rt_jl
