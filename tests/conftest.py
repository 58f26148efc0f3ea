import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run on the GPU box)")


@pytest.fixture(scope="session")
def golden_dir():
    return GOLDEN


@pytest.fixture(scope="session")
def pmc_dir(tmp_path_factory):
    """A PMC corpus directory holding the files of tests/golden/pmc_subset.tar.xz (make_pmc_subset.py)."""
    import tarfile
    d = tmp_path_factory.mktemp("pmc")
    with tarfile.open(os.path.join(GOLDEN, "pmc_subset.tar.xz")) as tf:
        for m in tf.getmembers():
            if m.isfile():
                (d / os.path.basename(m.name)).write_bytes(tf.extractfile(m).read())
    return str(d)


@pytest.fixture(scope="session")
def oracle_c():
    """ctypes handle on the plain-C oracle (built by oracle/Makefile)."""
    import ctypes
    import subprocess
    so = os.path.join(ROOT, "oracle", "_build", "liboracle.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    lib = ctypes.CDLL(so)
    lib.oracle_cosine_similarity.restype = ctypes.c_double
    return lib
