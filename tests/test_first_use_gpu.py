"""A hub launch as a process's first call into the library.  The hub kernels need more dynamic LDS than
the default limit, and each kernel family (csrc/srg_spmm.hip, csrc/srg_cheby.hip) raises the limit of its
own hub kernels at its first fork on a device; a family that launched before doing so would fail the
launch with a HIP error.  The rest of the suite cannot see that: its processes have long forked through
every family before most hub paths run.  So every case runs tests/first_use_cases.py in a fresh child
process, whose first library call is the hub launch; the child holds the result to the same call with
n_hub = 0, bit for bit, and the library's status to SRG_OK."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("case", ["cheby_hub_f64_w512", "cheby_hub_f64_w256", "spmm_cheby_f32", "spmm_csr_f32_hub_w256",
                                  "spmm_span_f32"])
def test_hub_launch_is_the_first_library_call(case):
    r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "first_use_cases.py"), case],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    assert f"first_use ok: {case}" in r.stdout.decode()
