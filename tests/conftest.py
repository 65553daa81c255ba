import os
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

REFERENCE = "/root/reference"
# the reference's own data fixtures the tests read (examples/example.heic, tests/data/*.heic, fuzzing/data/corpus/*.heic), stored under
# tests/golden/reference/ at the paths they have in the reference tree
REFERENCE_FIXTURES = os.path.join(ROOT, "tests", "golden", "reference")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def reference_dir():
    return REFERENCE_FIXTURES


@pytest.fixture(scope="session")
def reference_sources():
    """the reference's sources (its public headers), for the tests that compile against them"""
    if not os.path.isdir(REFERENCE):
        pytest.skip("reference tree not present on this machine")
    return REFERENCE
