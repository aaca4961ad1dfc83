"""Writes tests/golden/g10/expected.npz: two fixtures of score differences and what scikit-learn's LinearSVC makes of them, for the
tests of K23 (tests/test_svmfusion_cpu.py).  Needs scikit-learn (written with 1.7.2); the tests read the recorded arrays only.

    python tests/golden/g10/make_g10.py

Row t of a fixture D enters the fit as the reference's old/methods/sfusion.py:55-61 enters it: +D[t] with label +1 for even t, -D[t]
with label -1 for odd t.  Two fits per fixture: 'tight' = LinearSVC(C=0.01, dual=True, tol=1e-12, max_iter=10**6) and 'default' =
LinearSVC(C=0.01), the reference's own call."""
import os

import numpy as np
from sklearn.svm import LinearSVC

HERE = os.path.dirname(os.path.abspath(__file__))
C = 0.01


def fixture(rng, n, M):
    shift = np.linspace(0.4, -0.1, M)                                # the first models tell a like from a draw, the last do not
    return (rng.standard_normal((n, M)) * 0.5 + shift).astype(np.float32)


def fits(D):
    y = np.where(np.arange(len(D)) % 2 == 0, 1, -1).astype(np.int8)
    x = D * y[:, None].astype(np.float32)
    out = {}
    for name, clf in (('tight', LinearSVC(C=C, dual=True, tol=1e-12, max_iter=10 ** 6, random_state=0)),
                      ('default', LinearSVC(C=C, random_state=0))):
        clf.fit(x, y)
        out[name + '_coef'] = np.asarray(clf.coef_[0], dtype=np.float64)
        out[name + '_intercept'] = np.asarray(clf.intercept_, dtype=np.float64).reshape(1)
    return out


def main():
    rng = np.random.Generator(np.random.PCG64(10))
    arrays = {}
    for tag, (n, M) in (('a', (501, 3)), ('b', (64, 16))):
        D = fixture(rng, n, M)
        arrays['D_' + tag] = D
        for k, v in fits(D).items():
            arrays[k + '_' + tag] = v
    arrays['C'] = np.asarray([C])
    np.savez(os.path.join(HERE, 'expected.npz'), **arrays)
    for k, v in arrays.items():
        print(k, v.shape, v.dtype)


if __name__ == '__main__':
    main()
