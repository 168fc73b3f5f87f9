"""pytest configuration: the ``gpu`` marker (tests that need an MI355X; the CPU suite runs
``-m "not gpu"``), the repository root on ``sys.path`` and a temporary directory short enough for
unix sockets."""
import os
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


#: A unix socket's path holds at most 107 bytes (``sockaddr_un.sun_path``). The device-plugin and
#: process tests bind theirs up to ~65 bytes below ``tempfile.gettempdir()`` (``tmpXXXXXXXX/node-1/
#: device-plugins/nos-xcp-amd.com_spx_nps1.sock``; kubelet's own directory is short), so under a
#: temporary directory longer than this the suite moves its temporary files to a shorter one.
_TMP_MAX = 24
_TMP_CANDIDATES = ("/tmp", "/var/tmp", "/dev/shm")
_short_tmp = None
_tmpdir_env = os.environ.get("TMPDIR")


def _shorten_tempdir():
    global _short_tmp
    cur = tempfile.gettempdir()
    if len(cur) <= _TMP_MAX:
        return
    for cand in _TMP_CANDIDATES:
        if len(cand) < len(cur) and os.path.isdir(cand) and os.access(cand, os.W_OK | os.X_OK):
            _short_tmp = tempfile.mkdtemp(prefix="nos-", dir=cand)
            tempfile.tempdir = _short_tmp
            os.environ["TMPDIR"] = _short_tmp   # the processes the tests start
            return


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "slow: long-running simulation test")
    _shorten_tempdir()


def pytest_unconfigure(config):
    global _short_tmp
    if _short_tmp is not None:
        if tempfile.tempdir == _short_tmp:
            tempfile.tempdir = None
        if _tmpdir_env is None:
            os.environ.pop("TMPDIR", None)
        else:
            os.environ["TMPDIR"] = _tmpdir_env
        shutil.rmtree(_short_tmp, ignore_errors=True)
        _short_tmp = None


@pytest.fixture(autouse=True)
def _reset_known_geometries():
    from walkai_nos_amd.models.xcp import known_configs
    known_configs.reset_known_geometries()
    yield
    known_configs.reset_known_geometries()


#: GPU tests that measure how pod PROCESSES share the GPU run before every test that opens streams
#: in this pytest process: the kernel tests leave this process's CU-masked streams (hardware queues)
#: on the GPU, a node's agents hold none (they never open a GPU context), and queues of a process
#: that is not a pod perturb how the hardware deals the pods' queues over its pipes
#: (profiles/churn_probe_r6.json). The order within each group is kept.
_PROCESS_SHARING = ("share_compute_evenly", "share_one_gpu_evenly")


def pytest_collection_modifyitems(session, config, items):
    first = [it for it in items if any(k in it.nodeid for k in _PROCESS_SHARING)]
    if first:
        rest = [it for it in items if not any(k in it.nodeid for k in _PROCESS_SHARING)]
        items[:] = first + rest
