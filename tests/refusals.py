"""Shared by the modules that pin the launchers' argument checks (tests/test_gpu_edges_new_units.py,
tests/test_gpu_refusals.py): a context manager that expects an XclimHipError with a given code and message."""
import pytest

from xclim_amd._capi import XclimHipError


def raises(code, match):
    class Ctx:
        def __enter__(self):
            self.cm = pytest.raises(XclimHipError, match=match)
            self.info = self.cm.__enter__()
            return self

        def __exit__(self, *exc):
            done = self.cm.__exit__(*exc)
            assert self.info.value.code == code, self.info.value
            return done

    return Ctx()
