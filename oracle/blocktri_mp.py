"""ORACLE (test infrastructure, not product code) -- the linear solve of the position-tracking family's Newton step in mpmath, at 50
significant digits:

    K z = rhs,   K = blocktridiag(E_{t-1}^T, D_t + mu I, E_t)   symmetric, K[t, t+1] = E[t],

by plain block elimination, knot after knot (S_0 = D_0 + mu I, S_t = D_t + mu I - E_{t-1}^T S_{t-1}^{-1} E_{t-1}, y_t = rhs_t - E_{t-1}^T S_{t-1}^{-1}
y_{t-1}; back: z_t = S_t^{-1} (y_t - E_t z_{t+1})).  It shares no code with oracle/structured.py:block_tridiag_solve (block Cholesky in float64) nor
with the sweeps of csrc/oh_free.hip (serial Riccati, cyclic reduction, twisted factorisation).  The float64 entries of D, E and rhs are taken as
exact; before it returns, the solution's residual against the banded product is formed in the same precision and must be below 1e-40.

Only ``tests/`` may import it.
"""
import mpmath
import numpy as np

DPS = 50
RESIDUAL_MAX = "1e-40"


def _mat(A):
    mp = mpmath.mp
    return [[mp.mpf(float(v)) for v in row] for row in np.asarray(A, float)]


def _matvec(A, x, transpose=False):
    mp = mpmath.mp
    n = len(x)
    if transpose:
        return [mp.fsum(A[k][i] * x[k] for k in range(n)) for i in range(n)]
    return [mp.fsum(A[i][k] * x[k] for k in range(n)) for i in range(n)]


def _matmul(A, B, transpose_a=False):
    mp = mpmath.mp
    n = len(A)
    if transpose_a:
        return [[mp.fsum(A[k][i] * B[k][j] for k in range(n)) for j in range(n)] for i in range(n)]
    return [[mp.fsum(A[i][k] * B[k][j] for k in range(n)) for j in range(n)] for i in range(n)]


def _inverse(S):
    """S^{-1}: through the Cholesky factor where S is positive definite (every Schur complement of a positive definite K is; a third of the
    work of the general routine), else mp.inverse."""
    mp = mpmath.mp
    n = len(S)
    L = [[mp.zero] * n for _ in range(n)]
    for j in range(n):
        d = S[j][j] - mp.fsum(L[j][k] * L[j][k] for k in range(j))
        if not d > 0:
            return mp.inverse(mp.matrix(S)).tolist()
        L[j][j] = mp.sqrt(d)
        for i in range(j + 1, n):
            L[i][j] = (S[i][j] - mp.fsum(L[i][k] * L[j][k] for k in range(j))) / L[j][j]
    W = [[mp.zero] * n for _ in range(n)]  # L^{-1}, lower triangular
    for j in range(n):
        W[j][j] = 1 / L[j][j]
        for i in range(j + 1, n):
            W[i][j] = -mp.fsum(L[i][k] * W[k][j] for k in range(j, i)) / L[i][i]
    X = [[mp.zero] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1):
            X[i][j] = X[j][i] = mp.fsum(W[k][i] * W[k][j] for k in range(i, n))
    return X


def _is_diagonal(E):
    E = np.asarray(E)
    return not np.any(E[~np.eye(E.shape[0], dtype=bool)])


def solve_mp(D, E, rhs, mu, dps=DPS):
    """D: (N, m, m), E: (N-1, m, m), rhs: (N, m), mu: the shift on the diagonal.  -> (z as float64 (N, m), z in mpf [N][m], residual in mpf)."""
    mp = mpmath.mp
    with mp.workdps(dps):
        N, m = np.asarray(rhs).shape
        mu_mp = mp.mpf(float(mu))
        A = []
        for t in range(N):
            a = _mat(D[t])
            for i in range(m):
                a[i][i] += mu_mp
            A.append(a)
        Em = [_mat(E[t]) for t in range(N - 1)]
        r = [[mp.mpf(float(v)) for v in row] for row in np.asarray(rhs, float)]
        X, y = [], []
        S = A[0]
        for t in range(N):
            X.append(_inverse(S))
            if t == 0:
                y.append(r[0])
            if t < N - 1:
                if _is_diagonal(E[t]):  # (the family's coupling blocks: entry-wise, 49 products instead of 686)
                    e = [Em[t][i][i] for i in range(m)]
                    EXE = [[e[i] * X[t][i][j] * e[j] for j in range(m)] for i in range(m)]
                else:
                    EXE = _matmul(Em[t], _matmul(X[t], Em[t]), transpose_a=True)  # E_t^T S_t^{-1} E_t
                S = [[A[t + 1][i][j] - EXE[i][j] for j in range(m)] for i in range(m)]
                c = _matvec(Em[t], _matvec(X[t], y[t]), transpose=True)
                y.append([r[t + 1][i] - c[i] for i in range(m)])
        z = [None] * N
        for t in range(N - 1, -1, -1):
            v = y[t]
            if t < N - 1:
                c = _matvec(Em[t], z[t + 1])
                v = [v[i] - c[i] for i in range(m)]
            z[t] = _matvec(X[t], v)
        # the solution against the banded product
        res = mp.mpf(0)
        for t in range(N):
            kz = _matvec(A[t], z[t])
            if t > 0:
                c = _matvec(Em[t - 1], z[t - 1], transpose=True)
                kz = [kz[i] + c[i] for i in range(m)]
            if t < N - 1:
                c = _matvec(Em[t], z[t + 1])
                kz = [kz[i] + c[i] for i in range(m)]
            res = max(res, max(abs(kz[i] - r[t][i]) for i in range(m)))
        if not res <= mp.mpf(RESIDUAL_MAX):
            raise ArithmeticError(f"solve_mp: residual {mp.nstr(res, 5)} of the mpmath solution exceeds {RESIDUAL_MAX}")
        return np.array([[float(v) for v in row] for row in z]), z, res
