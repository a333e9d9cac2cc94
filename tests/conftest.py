import json
import os
import sys

# numpy's BLAS pool: one thread (set before numpy loads).  Its workers spin after every product; inside a CPU-quota
# cgroup on a many-core host that spinning gets the whole process parked by the kernel for tens of milliseconds --
# long enough for the evaluation server's 20 ms patience to run out under a test (see bench.py).
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")

import numpy as np  # noqa: E402
import pytest

# the oracle's OpenMP regions are small; on a many-core host the default team (one thread per core) costs more
# in start-up than it gains (the NDT oracle sets its own thread count per object)
os.environ.setdefault("OMP_NUM_THREADS", "16")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def pair():
    """Reference scan pair (ndt_omp/data/*.pcd) after the 0.1 m downsample of apps/align.cpp:60-69."""
    d = np.load(os.path.join(GOLDEN, "pair_0p1.npz"))
    return d["target"], d["source"]


@pytest.fixture(scope="session")
def reference_pcd(tmp_path_factory):
    """The reference's bundled scan pair as its raw PCD files (ndt_omp/data/251370668.pcd = target, 251371071.pcd =
    source; stored xz-compressed, byte for byte) -> (target path, source path)."""
    import lzma
    d = tmp_path_factory.mktemp("reference_pcd")
    paths = []
    for name in ("251370668", "251371071"):
        p = d / (name + ".pcd")
        p.write_bytes(lzma.open(os.path.join(GOLDEN, name + ".pcd.xz")).read())
        paths.append(str(p))
    return tuple(paths)


@pytest.fixture(scope="session")
def golden():
    with open(os.path.join(GOLDEN, "oracle_golden.json")) as f:
        return json.load(f)


@pytest.fixture(scope="session")
def golden_grid():
    return dict(np.load(os.path.join(GOLDEN, "grid_1p0.npz")))


@pytest.fixture(scope="session")
def built_lib():
    """The in-tree HIP library (cross-compiles without a GPU)."""
    from toyslam_amd import _lib
    _lib.build()
    return _lib.lib()


def rot_err(Ta, Tb):
    return float(np.abs(np.asarray(Ta)[:3, :3] - np.asarray(Tb)[:3, :3]).max())


def trans_err(Ta, Tb):
    return float(np.abs(np.asarray(Ta)[:3, 3] - np.asarray(Tb)[:3, 3]).max())


def run_ranks(cmds_envs, timeout=300):
    """Start one process per (argv, env), wait for all of them and return [(returncode, stdout, stderr)].  Whatever
    happens -- a rank failing before the rendezvous, the timeout, an exception here -- no child is left behind: the
    survivors are killed by PID (never by pattern) in the finally block."""
    import subprocess
    import tempfile
    import time
    procs, files = [], []
    try:
        for argv, env in cmds_envs:
            fo, fe = tempfile.TemporaryFile(), tempfile.TemporaryFile()  # files, not pipes: nobody has to drain them while we poll
            files.append((fo, fe))
            procs.append(subprocess.Popen(argv, env=env, stdout=fo, stderr=fe))
        t0 = time.monotonic()
        while any(p.poll() is None for p in procs):
            if any(p.poll() not in (None, 0) for p in procs):
                break  # a failed rank leaves its peers waiting in a collective for ever
            if time.monotonic() - t0 > timeout:
                break
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
    out = []
    for p, (fo, fe) in zip(procs, files):
        fo.seek(0)
        fe.seek(0)
        out.append((p.returncode, fo.read().decode("utf-8", "replace"), fe.read().decode("utf-8", "replace")))
        fo.close()
        fe.close()
    return out
