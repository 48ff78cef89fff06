"""csrc/copy_pool.hpp (the host half of the pinned staging ring under every large upload) on the CPU: tests/host/copy_pool_test.cpp
checks the plan of a transfer's pieces at the 256 KiB, 16 MiB and granule edges, a copy thread's share of a piece's rows over image
tables with empty images and row strides for every thread count from 1 to 16, and CopyPool::run over thousands of uneven jobs at 4
and 16 threads -- each against a plain loop of its own.  The program runs twice: as it is, and built with ThreadSanitizer, where the
pool's workers and the caller also exchange ordinary memory.  tests/test_upload_gpu.py runs the ring itself on the device."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("target", ["copy_pool_test", "copy_pool_test_tsan"])
def test_piece_plan_row_shares_and_copy_pool(target):
    subprocess.check_call(["make", "-C", os.path.join(HERE, "host"), target], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(HERE, "host", target)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "ThreadSanitizer" not in out.stderr and "ThreadSanitizer" not in out.stdout, out.stderr[-3000:]
    assert "plan: 84 combinations" in out.stdout and "shares: " in out.stdout and "pool: 2 x 3000 jobs, 100 lifetimes" in out.stdout
    assert "copy_pool_test: all checks passed" in out.stdout
