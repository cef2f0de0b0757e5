"""The reductions that hand one scalar to the host, and the two element-wise streams beside them, at the size edges of their kernels and against exact references.

Lengths: the wave (64), 256-thread and 1 024-thread workgroup boundaries, and two lengths derived from the device: grid_for caps a launch at 8·n_cu workgroups
of 256, grid_red at 2·n_cu of 1 024 — the same G = 8·n_cu·256 threads — so G + 1 and 2·G + 77 make the grid-stride loops take a second and a third trip with a
ragged tail.

References and tolerances:
  maxima        np.max of the addressed slice, asserted with ==: a maximum is exact (the sign of a zero result is not pinned).
  sums          inputs whose products are exact in double (significands of 24 bits, moderate exponents), so math.fsum of the products is the correctly
                rounded sum; the signs make it cancel to about 1e-8 of Σ|aᵢbᵢ|.  Tolerance (terms − 1)·2⁻⁵³·Σ|aᵢbᵢ|: the first-order bound of a recursive
                sum in ANY order (Higham, Accuracy and Stability of Numerical Algorithms, §4.2), the only thing a sum that ends in atomics promises.  Every
                |aᵢbᵢ| is at least 8 × that tolerance (asserted before the device is called): one dropped or doubled element fails.
  element-wise  k_heat_matrix and k_axpy are compiled with -ffp-contract=fast and the device code is one v_fma_f64 / v_fmac_f64 per element, in the
                paired body and in the odd tail alike: A = fma(−Δt, K, M) and y = fma(a, x, y), ONE rounding each.  The reference is therefore the exact
                rational M − Δt·K (a·x + y) rounded once, and the assertion is bit equality with it — not with NumPy's two roundings, from which it may
                differ by the rounding of Δt·K (a·x)."""
import ctypes as C
import fractions
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
FIXED = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099]
LENGTHS = FIXED + ["grid+1", "2grid+77"]
BOUNDARY = [64, 65, 256, 257, 1024, 1025, "grid+1"]          # where `*out += …` is checked twice over
FILL = 1.0e300                                                 # the rest of every allocation: larger in magnitude than anything addressed


def full_grid(device):
    """threads of one capped launch: 8·n_cu workgroups of 256 (grid_for) = 2·n_cu of 1 024 (grid_red)"""
    return 8 * device.info()["n_cu"] * 256


def length(device, n):
    G = full_grid(device)
    return {"grid+1": G + 1, "2grid+77": 2 * G + 77}.get(n, n)


def positions(device, n):
    """where the extreme element sits in turn: wave and workgroup edges, the last element, the first element of the second grid-stride trip"""
    return [p for p in dict.fromkeys([0, 63, 64, 255, 256, n - 1, full_grid(device)]) if 0 <= p < n]


def at(vec, index):
    return C.c_void_p(vec.data_ptr() + 8 * int(index))


def scalar(tb, fn, *args):
    out = C.c_double(-7.0)
    tb.check(fn(*args, C.byref(out)))
    return out.value


def poke(tb, device, vec, index, value):
    v = np.array([value], dtype=np.float64)
    tb.check(tb.lib().tb_memcpy_h2d(device.h, at(vec, index), v.ctypes.data_as(C.c_void_p), 8))


def strided(n, stride, phi, slice_values):
    """(allocation, offset): `slice_values` at offset + i·stride, FILL everywhere else — before, between and behind.  stride > 1 addresses state `phi`
    of a point-blocked array like _phi_slice does; stride 1 gets a guard element in front instead.  One full stride lies behind the last addressed
    element, so element n of an over-long read is a FILL value inside the allocation."""
    offset = phi if stride > 1 else 1
    buf = np.full(offset + (n - 1) * stride + 1 + stride, FILL)
    buf[offset:offset + (n - 1) * stride + 1:stride] = slice_values
    return buf, offset


def f24(x):
    """significand cut to 24 bits: products of two such numbers are exact in double"""
    return np.asarray(x, dtype=np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------- maxima
# every length at strides 1, 2 and 19 but 2·G + 77 at stride 19 (2·10⁷ doubles for nothing new: the third grid-stride trip runs at strides 1 and 2,
# stride 19 takes a second trip at G + 1)
MAX_CASES = [(n, stride, phi) for n in LENGTHS for stride, phi in ((1, 0), (2, 1), (19, 0)) if not (n == "2grid+77" and stride == 19)]


@pytest.mark.parametrize("n,stride,phi", MAX_CASES, ids=["%s-stride%d" % (n, s) for n, s, _ in MAX_CASES])
def test_max_and_absmax_read_exactly_the_addressed_slice(tb, device, n, stride, phi):
    n = length(device, n)
    lib = tb.lib()
    rng = np.random.default_rng(1000 * stride + n % 997)
    base = rng.uniform(-1.0, 1.0, n)
    buf, off = strided(n, stride, phi, base)
    d = device.to_device(buf)
    sl = buf[off:off + (n - 1) * stride + 1:stride]
    assert sl.size == n and np.abs(sl).max() <= 1.0 < FILL
    assert scalar(tb, lib.tb_max, device.h, n, at(d, off), stride) == np.max(sl)
    assert scalar(tb, lib.tb_absmax, device.h, n, at(d, off), stride) == np.max(np.abs(sl))
    for p in positions(device, n):
        for peak, fn, ref in ((2.0, lib.tb_max, np.max), (-3.0, lib.tb_absmax, lambda v: np.max(np.abs(v)))):
            poke(tb, device, d, off + p * stride, peak)
            sl[p] = peak
            got = scalar(tb, fn, device.h, n, at(d, off), stride)
            assert got == ref(sl) == abs(peak), (fn.__name__, n, stride, p, got)
            poke(tb, device, d, off + p * stride, base[p])
            sl[p] = base[p]


@pytest.mark.parametrize("n", [65, 257, 4099], ids=str)
def test_max_of_an_all_negative_slice_and_of_subnormals(tb, device, n):
    lib = tb.lib()
    rng = np.random.default_rng(n)
    tiny = 5e-324
    cases = {"negative": -rng.uniform(1.0, 2.0, n),                                         # signed max ≠ abs max
             "subnormal": rng.integers(1, 1000, n) * tiny * rng.choice([-1.0, 1.0], n),     # every value a subnormal, both signs
             "negative subnormal": -rng.integers(1, 1000, n) * tiny}
    for name, v in cases.items():
        for stride, phi in ((1, 0), (19, 0)):
            buf, off = strided(n, stride, phi, v)
            d = device.to_device(buf)
            got_max = scalar(tb, lib.tb_max, device.h, n, at(d, off), stride)
            got_abs = scalar(tb, lib.tb_absmax, device.h, n, at(d, off), stride)
            assert got_max == np.max(v) and got_abs == np.max(np.abs(v)), (name, stride, got_max, got_abs)
            if name.startswith("negative"):
                assert got_max < 0.0 < got_abs and got_max != -got_abs
            if "subnormal" in name:
                assert 0.0 < got_abs < 2.3e-308                                             # not flushed to zero


def test_max_of_nothing(tb, device):
    d = device.to_device(np.full(4, FILL))
    assert scalar(tb, tb.lib().tb_max, device.h, 0, d.ptr, 1) == -np.inf
    assert scalar(tb, tb.lib().tb_absmax, device.h, 0, d.ptr, 1) == 0.0


# ------------------------------------------------------------------------------------------- sums
def cancelling(mag):
    """Signs for terms of magnitudes mag[:-1] (multiples of 2⁻⁴⁵ below 8, so that every partial sum is exact) and the value of the last term, so that the
    sum of all is about 1e-8 of Σ|terms|: greedy signs keep the running sum below the largest term, the last but one term (magnitude 8, the caller's) moves
    it away from zero with the sign it has, and the last term closes it to the target.  Returns (signs of all but the last term, the last term)."""
    n = len(mag)
    s = np.ones(n - 1)
    run = 0.0
    for i in range(n - 2):
        s[i] = -1.0 if run > 0.0 else 1.0
        run += s[i] * mag[i]
    s[n - 2] = 1.0 if run >= 0.0 else -1.0
    run += s[n - 2] * mag[n - 2]
    return s, -run + 1e-8 * float(np.sum(mag[:-1]))


def dot_inputs(n, seed):
    """a, b with exact products, |aᵢbᵢ| in [1, 4) but for a closing pair: the elements come as pairs (s, −s) — and one triple (2s, −s, −s) where the count
    is odd — that cancel exactly, then +8 and −8 + 1e-8·Σ|aᵢbᵢ|, all of it shuffled, so that partners sit in different lanes, waves and workgroups"""
    rng = np.random.default_rng(seed)
    a, b = f24(rng.uniform(1.0, 2.0, n)), f24(rng.uniform(1.0, 2.0, n))
    if n < 5:
        return a, b * rng.choice([-1.0, 1.0], n)
    k = 0
    if n % 2:
        a[0:3] = (2.0, 1.0, 1.0)
        b[1] = b[2] = -b[0]
        k = 3
    m = (n - 2 - k) // 2
    a[k + m:k + 2 * m] = a[k:k + m]
    b[k + m:k + 2 * m] = -b[k:k + m]
    assert k + 2 * m == n - 2
    total = math.fsum(np.abs(a[:n - 2] * b[:n - 2])) + 16.0
    a[n - 2], b[n - 2] = 2.0, 4.0
    a[n - 1], b[n - 1] = 1.0, -8.0 + 1e-8 * total             # 1·b is exact whatever the significand of b
    perm = rng.permutation(n)
    return a[perm], b[perm]


def sum_reference(terms, nterms=None):
    """(correctly rounded sum, tolerance); asserts the terms are large enough for the tolerance to see one of them"""
    terms = np.asarray(terms, dtype=np.float64)
    nterms = terms.size if nterms is None else nterms
    ref = math.fsum(terms)
    sabs = math.fsum(np.abs(terms))
    tol = (nterms - 1) * U * sabs
    assert np.abs(terms).min() >= 2.0 ** -10 and np.abs(terms).min() >= 8.0 * tol, (np.abs(terms).min(), tol)
    if terms.size >= 63:
        assert abs(ref) <= 1e-7 * sabs, (ref, sabs)           # the sum does cancel: an absolute error of one term is 1e7 times the result
    return ref, tol


@pytest.mark.parametrize("n", LENGTHS, ids=str)
def test_dot_against_the_correctly_rounded_sum(tb, device, n):
    n = length(device, n)
    lib = tb.lib()
    a, b = dot_inputs(n, 5 * n + 1)
    ref, tol = sum_reference(a * b)                            # the products are exact, so a * b IS the list of terms
    da, db = device.to_device(a), device.to_device(b)
    got = scalar(tb, lib.tb_dot, device.h, n, da.ptr, db.ptr)
    print("tb_dot n=%d: device %.17g, fsum %.17g, |diff| %.3e, bound %.3e" % (n, got, ref, abs(got - ref), tol))
    assert abs(got - ref) <= tol
    # tb_cgd_dot: *out += Σ w·a·b in caller-owned device memory.  The weights are 1/k of a dof held by k ranks; with k a power of two a/w is exact and
    # w·(a/w)·b are the terms above, whichever way the kernel associates the product.
    w = np.random.default_rng(n).choice([1.0, 0.5, 0.25], n)
    daw, dw = device.to_device(a / w), device.to_device(w)
    assert np.array_equal(w * (a / w), a)
    calls = 2 if n in [length(device, m) for m in BOUNDARY] else 1
    for name, pw, pa in (("plain", None, da.ptr), ("weighted", dw.ptr, daw.ptr)):
        out = device.zeros(1)
        for _ in range(calls):
            tb.check(lib.tb_cgd_dot(device.h, n, pw, pa, db.ptr, out.ptr))
        got_w = out.to_host()[0]
        # (the second call adds its sum to the first one's: one more rounding, of the result)
        assert abs(got_w - calls * ref) <= calls * tol + (calls - 1) * U * abs(calls * ref), (name, n, calls, got_w, ref, tol)


def test_sums_of_nothing_leave_the_scalar(tb, device):
    lib = tb.lib()
    d = device.to_device(np.full(4, FILL))
    assert scalar(tb, lib.tb_dot, device.h, 0, d.ptr, d.ptr) == 0.0
    out = device.to_device(np.array([3.25]))
    tb.check(lib.tb_cgd_dot(device.h, 0, None, d.ptr, d.ptr, out.ptr))
    assert out.to_host()[0] == 3.25
    tb.check(lib.tb_axpy(device.h, 0, 2.0, d.ptr, d.ptr))
    assert np.array_equal(d.to_host(), np.full(4, FILL))


@pytest.fixture(scope="module")
def hex_patterns(tb, device):
    """the 5×4×3 and 14×12×10 perturbed hexahedral patterns of test_gpu_parity.py, with their device patterns"""
    out = {}
    for nel in ((5, 4, 3), (14, 12, 10)):
        g = tb.generate_mesh(tb.Hexahedron, nel, (0, 0, 0), (1.0, 1.0, 1.0), perturb=0.2)
        dh = tb.DofHandler(g)
        sp = tb.allocate_matrix(dh)
        M = tb.setup_operator(tb.PatchAssemblyStrategy(device), tb.BilinearMassIntegrator(tb.ConstantCoefficient(1.0)), dh, sp)
        out[nel] = (dh.ndofs, sp, M)
    return out


def row_of(sp):
    return np.repeat(np.arange(len(sp.rowptr) - 1), np.diff(sp.rowptr))


@pytest.mark.parametrize("nel", [(5, 4, 3), (14, 12, 10)], ids=["5x4x3", "14x12x10"])
def test_spmv_csr_dot_against_the_correctly_rounded_sum(tb, device, hex_patterns, nel):
    """*d_dot += xᵀ(A x): the terms xᵢ·Aᵢⱼ·xⱼ are exact with 12-bit x and 24-bit A.  The device rounds the row sums, their products with xᵢ and the sum of
    those, n·(entries of the longest row) operations at the very most: that many terms in the bound."""
    n, sp, M = hex_patterns[nel]
    lib = tb.lib()
    rng = np.random.default_rng(n)
    x = np.round(rng.uniform(1.0, 2.0, n) * 2048.0) / 2048.0 * rng.choice([-1.0, 1.0], n)     # 12 bits
    rows, cols = row_of(sp), sp.colidx
    last = sp.nnz - 1
    assert rows[last - 1] == rows[last]
    x[rows[last]] = x[cols[last]] = x[cols[last - 1]] = 1.0     # the two closing entries multiply 1·A·1: exact whatever their significands
    A = f24(rng.uniform(1.0, 2.0, sp.nnz))
    A[last - 1] = 8.0
    mag = np.abs(x[rows] * A * x[cols])
    signs, closing = cancelling(mag)
    A[:-1] *= signs * np.sign(x[rows[:-1]] * x[cols[:-1]])
    A[last] = closing
    terms = x[rows] * A * x[cols]
    ref, tol = sum_reference(terms, nterms=n * int(np.diff(sp.rowptr).max()))
    dA, dx, dy, out = device.to_device(A), device.to_device(x), device.zeros(n), device.zeros(1)
    for calls in (1, 2):
        tb.check(lib.tb_spmv_csr_dot(M.pattern.h, dA.ptr, dx.ptr, dy.ptr, out.ptr))
        got = out.to_host()[0]
        print("tb_spmv_csr_dot %s call %d: device %.17g, %d × fsum %.17g, bound %.3e" % (nel, calls, got, calls, ref, tol))
        assert abs(got - calls * ref) <= calls * tol + (calls - 1) * U * abs(calls * ref)    # (+ the rounding of the second call's addition)
    # y itself: every row sum within the any-order bound of its own terms
    y_ref = np.array([math.fsum(A[a:b] * x[cols[a:b]]) for a, b in zip(sp.rowptr[:-1], sp.rowptr[1:])])
    y_abs = np.add.reduceat(np.abs(A * x[cols]), sp.rowptr[:-1])
    assert np.all(np.abs(dy.to_host() - y_ref) <= (np.diff(sp.rowptr) - 1) * U * y_abs)


@pytest.mark.parametrize("nel", [(5, 4, 3), (14, 12, 10)], ids=["5x4x3", "14x12x10"])
def test_meandiag_of_a_diagonal_of_mixed_signs(tb, device, hex_patterns, nel):
    n, sp, M = hex_patterns[nel]
    rng = np.random.default_rng(3 * n)
    A = f24(rng.uniform(1.0, 2.0, sp.nnz)) * rng.choice([-1.0, 1.0], sp.nnz)
    diag = A[sp.colidx == row_of(sp)]
    assert diag.size == n and (diag < 0).any() and (diag > 0).any()
    sabs = math.fsum(np.abs(diag))
    ref = sabs / n
    tol = (n - 1) * U * sabs / n + 2.0 * U * ref                # the sum in any order, then the device's division and this one
    assert np.abs(diag).min() / n >= 8.0 * tol
    assert abs(math.fsum(diag)) < 0.5 * sabs                    # Σ d and Σ |d| are different numbers: a missing fabs is seen
    dA = device.to_device(A)
    got = scalar(tb, tb.lib().tb_meandiag, M.pattern.h, dA.ptr)
    print("tb_meandiag %s: device %.17g, fsum(|d|)/n %.17g, bound %.3e" % (nel, got, ref, tol))
    assert abs(got - ref) <= tol


# ------------------------------------------------------------------------------------------- element-wise streams
def fma_rounded(a, x, y):
    """a·x + y of every element with ONE rounding: exact rational arithmetic, rounded to nearest-even by float()"""
    F = fractions.Fraction
    return np.array([float(F(a) * F(float(xi)) + F(float(yi))) for xi, yi in zip(x, y)])


@pytest.mark.parametrize("n", FIXED, ids=str)
def test_heat_matrix_and_axpy_are_one_fma_per_element(tb, device, n):
    """odd lengths run the scalar tail of k_heat_matrix (its body handles pairs), even ones do not"""
    lib = tb.lib()
    rng = np.random.default_rng(n)
    m, k = rng.normal(size=n), rng.normal(size=n) * 10.0 ** rng.integers(-3, 4, n)
    dt = 0.3
    guard = 3                                                   # elements behind the end: must stay as they are
    out = device.to_device(np.full(n + guard, FILL))
    dm, dk = device.to_device(m), device.to_device(k)
    tb.check(lib.tb_heat_matrix(device.h, n, dm.ptr, dk.ptr, dt, out.ptr))
    got = out.to_host()
    ref = fma_rounded(-dt, k, m)
    assert np.array_equal(got[:n].view(np.uint64), ref.view(np.uint64)), (n, np.flatnonzero(got[:n] != ref)[:5])
    assert np.all(got[n:] == FILL)
    x, y = rng.normal(size=n), rng.normal(size=n)
    dy = device.to_device(np.concatenate([y, np.full(guard, FILL)]))
    dx = device.to_device(x)
    tb.check(lib.tb_axpy(device.h, n, -1.7, dx.ptr, dy.ptr))
    got = dy.to_host()
    ref = fma_rounded(-1.7, x, y)
    assert np.array_equal(got[:n].view(np.uint64), ref.view(np.uint64)), (n, np.flatnonzero(got[:n] != ref)[:5])
    assert np.all(got[n:] == FILL)
