import os
import pathlib
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (gfx950) GPU")
    config.addinivalue_line("markers", "slow: long-running test")


@pytest.fixture
def sock_dir():
    """A private directory for unix sockets whose path is short enough for sockaddr_un
    (108 bytes with the socket's name) wherever pytest's own temporary directory lies."""
    import shutil
    import tempfile
    longest = len("/skXXXXXXXX/selkies_event1000.sock")
    for base in (tempfile.gettempdir(), "/tmp", "/var/tmp", "/dev/shm"):
        if len(base) + longest < 108 and os.path.isdir(base) and os.access(base, os.W_OK | os.X_OK):
            break
    else:
        pytest.fail("no writable directory with a path short enough for a unix socket")
    d = tempfile.mkdtemp(prefix="sk", dir=base)
    yield pathlib.Path(d)
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="session")
def native_lib():
    from selkies_gstreamer_amd.ops import native
    return native.lib()
