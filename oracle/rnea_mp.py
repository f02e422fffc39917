"""ORACLE (test infrastructure, not product code) -- RobotModel.rnea (models.py:1819-1880) restated one sample at a time in mpmath, at 50
significant digits, from the numpy restatement oracle/torque.py:rnea_batch and its RneaTables.

Derivatives come from finite differences in the high precision, so nothing here shares code with the kernels' dual numbers, their hand-written
adjoint (csrc/oh_rnea.h:rnea_ctau_grad_inv) or the complex-step oracle (oracle/torque.py:rnea_jacobian, rnea_ctau_hessian, which
differentiate rnea_batch and a hand-written numpy adjoint):
  J = d tau / d (q, qd, qdd)   central differences, h = 1e-15: truncation ~ h^2 = 1e-30, rounding ~ 1e-50 / h = 1e-35;
  H = d^2 (c^T tau) / dz^2     4-point mixed (and 3-point diagonal) differences, h = 1e-12: truncation ~ 1e-24, rounding ~ 1e-50 / h^2 = 1e-26.
Both are rounded to float64 at the end.  The tables are the float64 numbers RneaTables holds, taken as exact.

Only ``tests/`` may import it.
"""
import mpmath
import numpy as np

DPS = 50
H_JAC = "1e-15"
H_HESS = "1e-12"


class MpTables:
    """RneaTables in mpf (exact images of the float64 entries)."""

    def __init__(self, tb):
        mp = mpmath.mp
        self.n, self.ndof = tb.n, tb.ndof
        f = lambda a: [mp.mpf(float(x)) for x in np.asarray(a, float).reshape(-1)]
        self.m = f(tb.m)
        self.cm = [f(v) for v in tb.cm]
        self.I = [f(M) for M in tb.I]  # row-major 3 x 3
        self.xyz = [f(v) for v in tb.xyz]
        self.R0 = [f(M) for M in tb.R0]
        self.axis = [f(v) for v in tb.axis]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _mv(M, v):  # M v, M row-major 3 x 3
    return [M[3 * i] * v[0] + M[3 * i + 1] * v[1] + M[3 * i + 2] * v[2] for i in range(3)]


def _mtv(M, v):  # M^T v
    return [M[i] * v[0] + M[3 + i] * v[1] + M[6 + i] * v[2] for i in range(3)]


def _mm(A, B):
    return [sum(A[3 * i + k] * B[3 * k + j] for k in range(3)) for i in range(3) for j in range(3)]


def _add(*vs):
    return [sum(c) for c in zip(*vs)]


def _scale(s, v):
    return [s * x for x in v]


def tau_mp(mt: MpTables, q, qd, qdd):
    """tau (list of ndof mpf) at one sample; q, qd, qdd: sequences of mpf (or floats, taken exactly)."""
    mp = mpmath.mp
    n = mt.n
    zero = [mp.zero] * 3
    om, omD, vD = zero, zero, [mp.zero, mp.zero, mp.mpf("9.81")]
    Rs, fs, ns = [], [], []
    for i in range(n):
        if i != n - 1:
            s, c = mp.sin(q[i]), mp.cos(q[i])
            k = mt.axis[i]
            K = [0, -k[2], k[1], k[2], 0, -k[0], -k[1], k[0], 0]
            KK = _mm(K, K)
            Rq = [(1 if r in (0, 4, 8) else 0) + s * K[r] + (1 - c) * KK[r] for r in range(9)]
            R = _mm(mt.R0[i], Rq)  # pRi
        else:
            R = mt.R0[i]
        Rs.append(R)
        omp, omDp = _mtv(R, om), _mtv(R, omD)
        if i != n - 1:
            a = _mtv(R, mt.axis[i])
            aq = _scale(qd[i], a)
            omi = _add(omp, aq)
            omDi = _add(omDp, _cross(omp, aq), _scale(qdd[i], a))
        else:
            omi, omDi = omp, omDp
        r = mt.xyz[i]
        vDi = _mtv(R, _add(vD, _cross(omD, r), _cross(om, _cross(om, r))))
        cm = mt.cm[i]
        fs.append(_scale(mt.m[i], _add(vDi, _cross(omDi, cm), _cross(omi, _cross(omi, cm)))))
        ns.append(_add(_mv(mt.I[i], omDi), _cross(omi, _mv(mt.I[i], omi))))
        om, omD, vD = omi, omDi, vDi
    ifi = fs[n - 1]
    ini = _add(ns[n - 1], _cross(mt.cm[n - 1], fs[n - 1]))
    taus = [None] * (n - 1)
    for i in range(n - 1, 0, -1):
        R = Rs[i]
        Rf = _mv(R, ifi)
        ini = _add(ns[i - 1], _mv(R, ini), _cross(mt.cm[i - 1], fs[i - 1]), _cross(mt.xyz[i], Rf))
        ifi = _add(Rf, fs[i - 1])
        a = _mtv(Rs[i - 1], mt.axis[i - 1])
        taus[i - 1] = ini[0] * a[0] + ini[1] * a[1] + ini[2] * a[2]
    return taus


def _split(mt, z):
    nd = mt.ndof
    return z[:nd], z[nd:2 * nd], z[2 * nd:]


def _mpz(*parts):
    return [mpmath.mp.mpf(float(x)) for p in parts for x in np.asarray(p, float).reshape(-1)]


def rnea_mp(tb, q, qd, qdd):
    """tau at one sample (float64 arrays in, float64 out)."""
    with mpmath.workdps(DPS):
        mt = MpTables(tb)
        return np.array([float(t) for t in tau_mp(mt, *_split(mt, _mpz(q, qd, qdd)))])


def rnea_jacobian_mp(tb, q, qd, qdd):
    """d tau / d (q, qd, qdd) at one sample: (ndof, 3 ndof)."""
    with mpmath.workdps(DPS):
        mp = mpmath.mp
        mt = MpTables(tb)
        z = _mpz(q, qd, qdd)
        h = mp.mpf(H_JAC)
        J = np.empty((mt.ndof, len(z)))
        for d in range(len(z)):
            zp, zm = list(z), list(z)
            zp[d] += h
            zm[d] -= h
            tp, tm = tau_mp(mt, *_split(mt, zp)), tau_mp(mt, *_split(mt, zm))
            for i in range(mt.ndof):
                J[i, d] = float((tp[i] - tm[i]) / (2 * h))
        return J


def rnea_ctau_hessian_mp(tb, q, qd, qdd, c):
    """sum_i c_i d^2 tau_i / d (q, qd, qdd)^2 at one sample: (3 ndof, 3 ndof), every entry differenced (zero blocks included)."""
    with mpmath.workdps(DPS):
        mp = mpmath.mp
        mt = MpTables(tb)
        z = _mpz(q, qd, qdd)
        cc = _mpz(c)
        h = mp.mpf(H_HESS)
        nz = len(z)

        def f(*steps):
            zz = list(z)
            for d, s in steps:
                zz[d] += s * h
            return mp.fsum(ci * ti for ci, ti in zip(cc, tau_mp(mt, *_split(mt, zz))))

        f0 = f()
        H = np.empty((nz, nz))
        for a in range(nz):
            H[a, a] = float((f((a, 1)) - 2 * f0 + f((a, -1))) / (h * h))
            for b in range(a + 1, nz):
                v = (f((a, 1), (b, 1)) - f((a, 1), (b, -1)) - f((a, -1), (b, 1)) + f((a, -1), (b, -1))) / (4 * h * h)
                H[a, b] = H[b, a] = float(v)
        return H
