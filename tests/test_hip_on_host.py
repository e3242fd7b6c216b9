"""tests/cpp/hip_on_host, the stand-in <hip/hip_runtime.h> that the *_on_host tests run the library's kernels through, held to
plain definitions by tests/cpp/hip_on_host_check.cpp: the arithmetic stand-ins over all byte pairs and the table that
csrc/lfg_device.hpp records, a launch's indices, every cross-lane primitive with all lanes live and with lanes that have
returned, the barrier and the atomics.  A wrong stand-in makes every result behind it worthless, so this comes first.  Built
plainly and with -fsanitize=address,undefined.  CPU only."""
import subprocess

import pytest

from tests import on_host_kit as kit


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    return kit.build(tmp_path_factory, request.param, "hip_on_host_check", [])


def test_every_stand_in_equals_its_plain_definition(program):
    p = subprocess.run([str(program)], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    assert p.stdout.startswith("ok "), p.stdout
