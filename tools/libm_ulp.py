"""Largest error, in units in the last place, of the device math library's expf and logf against float64 -- the two constants
EXPF_ULP / LOGF_ULP of tests/loss_f64_ref.py (the bound of csrc/lovasz.hip's cross-entropy and KL kernels).

    python tools/libm_ulp.py --build-only        # compile tools/libm_ulp.hip with the library's flags (no GPU needed)
    python tools/libm_ulp.py                     # the sweep, on the GPU

The sweep is exhaustive over the arguments the loss kernels can pass: every fp32 value in [-104, -2^-30] for expf (x - max <= 0;
below -104 the result is 0, above -2^-30 it rounds to 1), every fp32 value in [1, 256] for logf (the sum of C <= 256 terms of
which the largest is 1).  The float64 reference is torch's exp / log of the same values in float64 on the device (their own
error, a few 1e-16 relative, is 1e-8 of an fp32 unit in the last place).  An error is measured in units of the last place OF
THE REFERENCE VALUE; results below 2^-126 (subnormal) are reported apart, in units of 2^-149."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SRC = os.path.join(ROOT, 'tools', 'libm_ulp.hip')
LIB = os.path.join(ROOT, 'build', 'libm_ulp.so')
CHUNK = 1 << 24


def build():
    from u2mkd_amd import build as b
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
        subprocess.run([b.HIPCC, *b.FLAGS, '-shared', SRC, '-o', LIB], check=True)
    return LIB


def sweep(lib, which, lo_bits, hi_bits):
    """every fp32 value whose bit pattern lies in [lo_bits, hi_bits]: (largest error in ulp of a normal result, its argument,
    largest error of a subnormal result in units of 2^-149, values seen)"""
    import torch
    worst, at, worst_sub, seen = 0.0, None, 0.0, 0
    for b0 in range(lo_bits, hi_bits + 1, CHUNK):
        n = min(CHUNK, hi_bits + 1 - b0)
        bits = torch.arange(b0, b0 + n, dtype=torch.int64, device='cuda')
        x = (bits - (1 << 32) * (bits >= (1 << 31))).to(torch.int32).view(torch.float32)
        y = torch.empty_like(x)
        rc = lib.libm_apply(x.data_ptr(), n, which, y.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        ref = torch.exp(x.double()) if which == 0 else torch.log(x.double())
        err = (y.double() - ref).abs()
        normal = ref.abs() >= 2.0 ** -126
        expo = torch.frexp(ref.abs().clamp(min=2.0 ** -126))[1] - 1                # floor(log2 |ref|)
        ulp = torch.ldexp(torch.ones_like(ref), expo - 23)
        r = torch.where(normal, err / ulp, torch.zeros_like(err))
        zero = ref == 0                                                         # logf(1) = 0: the result has to be 0
        r = torch.where(zero, torch.where(y == 0, 0.0, float('inf')).to(r.dtype), r)
        k = int(r.argmax())
        if float(r[k]) > worst:
            worst, at = float(r[k]), float(x[k])
        sub = torch.where(~normal & ~zero, err / 2.0 ** -149, torch.zeros_like(err))
        worst_sub = max(worst_sub, float(sub.max()))
        seen += n
    return worst, at, worst_sub, seen


def f32_bits(v):
    import struct
    return struct.unpack('<I', struct.pack('<f', v))[0]


def main():
    path = build()
    if '--build-only' in sys.argv:
        print(path)
        return
    import torch                                   # first: the probe has to bind to the HIP runtime torch has loaded
    torch.cuda.init()
    lib = ctypes.CDLL(path)
    lib.libm_apply.restype = ctypes.c_int
    lib.libm_apply.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    # negative floats: the bit pattern grows with the magnitude
    w, at, ws, n = sweep(lib, 0, f32_bits(-2.0 ** -30), f32_bits(-104.0))
    print('LIBM expf  [-104, -2^-30]  %d values  max error %.4f ulp at x = %r  (subnormal results: %.4f units of 2^-149)' % (n, w, at, ws))
    w, at, ws, n = sweep(lib, 1, f32_bits(1.0), f32_bits(256.0))
    print('LIBM logf  [1, 256]        %d values  max error %.4f ulp at x = %r' % (n, w, at))


if __name__ == '__main__':
    main()
