"""The m = 0 reduction as both host drivers call it (csrc/mom_reduce.hpp): tests/host/reduce_check.cpp, built with the host
compiler under the address and undefined-behaviour sanitizers and run as a child process, against the same verdicts and cuts
computed in numpy from the index rule full(i0) = (i0 // 2) nS + i0 % 2.  Exact comparison: the cut only moves numbers."""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "radiativetransfer.jl_amd" / "csrc"


@pytest.fixture(scope="module")
def reduce_check(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("reduce") / "reduce_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(CSRC), str(ROOT / "tests" / "host" / "reduce_check.cpp"), "-o", str(exe)], check=True)

    def run(I0, mu, wt, Zpp, Zmp, Rsurf, nS, N0):
        N, _, K, M = Zpp.shape
        text = " ".join([f"{N} {nS} {K} {M} {N0}"] + [" ".join(repr(float(x)) for x in np.ravel(a, order="F"))
                                                     for a in (I0, mu, wt, Zpp, Zmp, Rsurf)])
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr  # a sanitizer report ends the program with a non-zero status
        res = {}
        for line in out.stdout.splitlines():
            name, *vals = line.split()
            res[name] = np.array([float(v) for v in vals])
        return res
    return run


def scene(nS, N, K=2, M=2, seed=0):
    """Random streams, bases and BRDF matrix whose moment-0 blocks do not couple (I,Q) with (U,V); the moment-1 blocks do."""
    rng = np.random.default_rng(seed)
    mu, wt = rng.uniform(0.1, 1.0, N), rng.uniform(0.1, 1.0, N)
    Zpp, Zmp = rng.normal(size=(N, N, K, M)), rng.normal(size=(N, N, K, M))
    Rsurf = rng.normal(size=(N, N))
    c = coupling(N, nS)
    Zpp[c, :, 0] = 0.0
    Zmp[c, :, 0] = 0.0
    Rsurf[c] = 0.0
    I0 = np.array([1.0, 0.25, 0.0, 0.0])
    return I0, mu, wt, Zpp, Zmp, Rsurf


def coupling(N, nS):
    iq = (np.arange(N) % nS) < 2
    return iq[:, None] != iq[None, :]


def numpy_reduction(I0, mu, wt, Zpp, Zmp, Rsurf, nS, N0):
    N, _, K, _ = Zpp.shape
    c = coupling(N, nS)
    N0r = 2 * (N // nS)
    full = [(i0 // 2) * nS + i0 % 2 for i0 in range(N0r)]
    ref = {"reducible": float(np.all(I0[2:nS] == 0.0) and not np.any(Zpp[c, :, 0] != 0.0) and not np.any(Zmp[c, :, 0] != 0.0)),
           "brdf": float(not np.any(Rsurf[c] != 0.0))}
    for name, src, dummy in (("mu", mu, 1.0), ("wt", wt, 0.0)):
        ref[name] = np.full(N0, dummy)
        ref[name][:N0r] = src[full]
    ref["sg"] = np.ones(N0)
    for name, Z in (("Zpp", Zpp), ("Zmp", Zmp)):
        cut = np.zeros((N0, N0, K))
        cut[:N0r, :N0r, :] = Z[:, :, :, 0][np.ix_(full, full)]
        ref[name] = cut.ravel(order="F")
    r0 = np.zeros((N0, N0))
    r0[:N0r, :N0r] = Rsurf[np.ix_(full, full)]
    ref["r0"] = r0.ravel(order="F")
    return ref


def check(reduce_check, case, nS, N0, reducible, brdf=True):
    got, ref = reduce_check(*case, nS, N0), numpy_reduction(*case, nS, N0)
    assert ref["reducible"] == float(reducible) and ref["brdf"] == float(brdf)  # the case is what its name says
    assert got["reducible"] == ref["reducible"] and got["brdf"] == ref["brdf"]
    for name in ("mu", "wt", "sg", "Zpp", "Zmp") + (("r0",) if brdf else ()):
        assert got[name].shape == ref[name].shape and np.array_equal(got[name], ref[name]), name


@pytest.mark.parametrize("nS,N,N0", [(3, 6, 4), (3, 6, 8), (4, 8, 4)])  # N0 = 8: four dummy entries behind the N0r = 4 real ones
def test_cut_matches_the_index_rule(reduce_check, nS, N, N0):
    check(reduce_check, scene(nS, N), nS, N0, reducible=True)  # (the BRDF matrix is block-structured: its cut matches too)


def test_coupling_in_moment_1_only_is_reducible(reduce_check):
    I0, mu, wt, Zpp, Zmp, Rsurf = scene(3, 6)
    c = coupling(6, 3)
    Zpp[c, :, 1] = 0.0
    Zmp[c, :, 1] = 0.0
    Zmp[2, 0, 1, 1] = 0.5  # U <- I, basis 1, moment 1
    check(reduce_check, (I0, mu, wt, Zpp, Zmp, Rsurf), 3, 4, reducible=True)


def test_coupling_in_moment_0_of_one_basis_is_not_reducible(reduce_check):
    I0, mu, wt, Zpp, Zmp, Rsurf = scene(3, 6)
    Zmp[2, 0, 1, 0] = 0.5  # U <- I, basis 1 of Zmp only, moment 0
    check(reduce_check, (I0, mu, wt, Zpp, Zmp, Rsurf), 3, 4, reducible=False)


def test_polarised_source_is_not_reducible(reduce_check):
    I0, mu, wt, Zpp, Zmp, Rsurf = scene(3, 6)
    I0[2] = 0.125
    check(reduce_check, (I0, mu, wt, Zpp, Zmp, Rsurf), 3, 4, reducible=False)


def test_coupling_brdf_is_refused(reduce_check):
    I0, mu, wt, Zpp, Zmp, Rsurf = scene(3, 6)
    Rsurf[5, 3] = 0.5  # U of stream 1 <- I of stream 1
    check(reduce_check, (I0, mu, wt, Zpp, Zmp, Rsurf), 3, 4, reducible=True, brdf=False)
