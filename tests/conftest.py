import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden():
    import glob
    import numpy as np

    class _Parts:
        """a fixture stored as <name>.part0.npz, <name>.part1.npz, ... (every committed file stays under 1 MiB); reads like
        the single .npz: g[key], key in g.files"""
        def __init__(self, paths):
            self._of = {k: z for z in (np.load(p) for p in paths) for k in z.files}
            self.files = list(self._of)

        def __getitem__(self, key):
            return self._of[key][key]

    class _G:
        def __init__(self):
            self._f = {}

        def __call__(self, name):
            if name not in self._f:
                path = os.path.join(GOLDEN, name + ".npz")
                parts = sorted(glob.glob(os.path.join(GOLDEN, glob.escape(name) + ".part*.npz")))
                self._f[name] = _Parts(parts) if parts and not os.path.exists(path) else np.load(path)
            return self._f[name]
    return _G()


@pytest.fixture(scope="session")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")
