"""The three-operation quotient of the fp32 step (csrc/dev_math.inc, DevMathF::quot) on the device -- needs an MI355X.

quot(a, b, y1) = fma(fma(-b, a*y1, a), y1, a*y1) is the correctly rounded a / b when y1 is the correctly rounded reciprocal
of b (the argument stands at DevMathF::quot).  Two things are checked here, both as conditions, not tolerances:
the device's refined reciprocal IS the correctly rounded one for every significand (the library's compiled-in set of
exceptions is empty), and the quotient has the bits of the device's IEEE division over structured operands.  The step
itself is covered by the parity tests, which compare every output with the reference bit for bit."""
import ctypes as C

import numpy as np
import pytest

from troute_amd import _lib

pytestmark = pytest.mark.gpu

RCP_EXCEPTIONS = ()   # the significands compiled in as excepted: none (DevMathF::quot, hypothesis (1))


@pytest.mark.parametrize("exponent", [-14, 0, 35])
def test_refined_reciprocal_is_correctly_rounded_for_every_significand(exponent):
    """All 2**23 significands of one binade inside the proved divisor ranges: the device's refined_rcp against the host's
    correctly rounded reciprocal, float32(1 / float64(b)) -- exact, fp64 carries more than 2*24 + 2 bits.  The set of
    mismatching significands must equal the compiled-in exception set; the device's own count (what = 2, against its fp64
    division) must say the same."""
    lib = _lib.lib()
    n = 1 << 23
    got = np.empty(n, np.float32)
    _lib.check(lib.trmc_selfcheck_rcp_values(0, exponent, got.ctypes.data_as(C.c_void_p)))
    b = ((np.uint32(exponent + 127) << np.uint32(23)) | np.arange(n, dtype=np.uint32)).view(np.float32)
    want = (1.0 / b.astype(np.float64)).astype(np.float32)
    differ = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    print(f"exponent {exponent}: {differ.size} significands differ", [hex(int(s)) for s in differ[:16]])
    assert tuple(int(s) for s in differ) == RCP_EXCEPTIONS
    checked, bad = C.c_int64(0), C.c_int64(-1)
    _lib.check(lib.trmc_selfcheck_fast_arith(0, 2, exponent, 0, C.byref(checked), C.byref(bad)))
    assert checked.value == n and bad.value == len(RCP_EXCEPTIONS), (checked.value, bad.value)


def test_quotient_has_the_bits_of_the_division():
    """65 666 divisors (2**16 significands at a stride of 128, every one within 64 of 0 and of 2**23 - 1; no exception has a
    neighbourhood to add) x 4 096 numerators each -- random significands at every exponent distance in [-40, 50], and
    a = b*q +- 1 ulp for q next to a rounding boundary (...0111..., ...1000...) -- and the numerator +0, which must give +0:
    2.7 x 10**8 pairs in one launch, compared on the device with its IEEE division.  No mismatch is allowed."""
    lib = _lib.lib()
    checked, bad = C.c_int64(0), C.c_int64(-1)
    _lib.check(lib.trmc_selfcheck_fast_arith(0, 3, 4096, 1, C.byref(checked), C.byref(bad)))
    print(f"{checked.value} pairs, {bad.value} mismatches")
    assert checked.value == 65666 * 4097 and bad.value == 0, (checked.value, bad.value)


def test_quotient_has_the_bits_of_the_division_over_the_operands_of_the_coefficients():
    """The same over DevMathF::div4's own operand box (what = 4), which the test above does not reach: the 65 666 divisors at
    exponents in [-21, 52], each with 4 096 numerators of both signs at absolute magnitudes -- 2**-60 .. 2**60 (ql*dt), 2**-45 ..
    2**52 (the two differences), 2**-21 .. 2**52 (the sum): exponent distances from -112 to +81, past the 2**96 inside which the
    compiler's division needs no scaling -- half of them a = d*q +- 1 ulp for q of either sign next to a rounding boundary; and
    the numerators +0 and -0 through div4 under coef_guard's verdict, which must give the zeros of the IEEE division (-0 is what
    a negative ql*dt that underflows becomes: it has to fail the guard).  No mismatch is allowed."""
    lib = _lib.lib()
    checked, bad = C.c_int64(0), C.c_int64(-1)
    _lib.check(lib.trmc_selfcheck_fast_arith(0, 4, 4096, 1, C.byref(checked), C.byref(bad)))
    print(f"{checked.value} pairs, {bad.value} mismatches")
    assert checked.value == 65666 * 4098 and bad.value == 0, (checked.value, bad.value)
