"""CPU numerics that every x86-64 host reproduces bit for bit, for fixtures compared at fp32 round-off.

MKL picks its kernels by CPU vendor and instruction set, ATen its vectorised kernels by instruction set, and both split
reductions by thread count; a deep network with hard window / quantiser edges turns those last-place differences into
logit changes far above round-off on another host.  ``ENV`` pins all three: MKL's conditional-numerical-reproducibility
path for any Intel-compatible CPU, ATen's AVX2 kernels and four threads.  MKL and ATen read these settings once per
process, so the computation runs in a child process; tests/golden/make_golden.py (``pinned``) writes the reference's side
of the comparison under the same settings."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = {'MKL_CBWR': 'COMPATIBLE', 'ATEN_CPU_CAPABILITY': 'avx2', 'OMP_NUM_THREADS': '4', 'MKL_NUM_THREADS': '4'}


def run(code, out, timeout=600):
    """Run the Python ``code`` (which saves its arrays with ``np.savez(OUT, ...)``) under ENV; returns the arrays."""
    prelude = 'import sys; sys.path.insert(0, %r); OUT = %r\n' % (ROOT, str(out))
    r = subprocess.run([sys.executable, '-c', prelude + code], env=dict(os.environ, **ENV), capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    with np.load(out) as f:
        return dict(f)
