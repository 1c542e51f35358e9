"""The built kernel library exports every entry point the Python side binds.

``ops._native._load()`` skips a name in ``_SIGS`` that the library lacks (alternative builds
selected by ``O3S_KERNEL_LIB`` may be older), so an entry point lost in a move between
``csrc/*.hip`` files would surface only at its first call.  These tests look at the library
built from this tree.  No GPU is needed: the library loads without one.
"""
import ctypes

import pytest

from orange3_spark_amd.ops import _native as N
from orange3_spark_amd.ops import build as B


@pytest.fixture(scope="module")
def built_lib():
    N.kernels()   # builds the library if it is missing
    return ctypes.CDLL(str(B.KERNEL_LIB))


def test_every_bound_entry_point_is_exported(built_lib):
    missing = [name for name in N._SIGS if not hasattr(built_lib, name)]
    assert not missing, missing


def test_every_preload_tag_has_its_entry_point(built_lib):
    missing = [tag for tag in N.PRELOAD_TAGS if not hasattr(built_lib, f"o3s_preload_{tag}")]
    assert not missing, missing


def test_every_kernel_file_has_a_preload_tag():
    stems = {p.stem for p in B.CSRC.glob("*.hip")}
    assert stems and stems <= set(N.PRELOAD_TAGS), sorted(stems - set(N.PRELOAD_TAGS))
