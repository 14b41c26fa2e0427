"""The dense layer blocks without a GPU: the library's entry points and the column sum's
workspace size, and the flagged-row counts of tests/test_gpu_dense.py's constant-input cases."""
import numpy as np
import torch

import mmgcn_ref as R


def test_library_symbols_and_limits():
    from rsx import _lib as L

    lib = L.lib()
    for name in ("rsx_dense_gemm", "rsx_dense_normalize_fwd", "rsx_dense_normalize_bwd", "rsx_dense_colsum_ws_bytes",
                 "rsx_dense_colsum", "rsx_dense_leaky_bwd"):
        assert hasattr(lib, name) and name in L.EXPORTED, name
    assert lib.rsx_dense_colsum_ws_bytes(1001, 256) == 8 * 256 * 4


def test_constant_input_cases_flag_few_rows():
    """The rows whose float64 pre-activation comes near leaky_relu's kink, for the generator and
    the draws of test_gpu_dense.test_wide_product_on_a_constant_input_vs_float64: 1, 0, 0, 2 and
    13 rows, at most 1.6 % (the GPU test's cap is 5 %)."""
    cases = [(4, 32, 65), (36, 64, 5), (36, 64, 65), (36, 32, 1001), (100, 256, 1001)]
    flagged = []
    for K, N, n in cases:
        rng = np.random.default_rng(1000 + K + N + n)
        f32 = lambda a: torch.from_numpy(a.astype(np.float32)).double()  # noqa: E731
        x = f32(rng.standard_normal((n, K)) * 0.5)
        B = f32(rng.standard_normal((N, K)) / np.sqrt(K))
        b = f32(rng.standard_normal(N) * 0.1)
        flagged.append(int(R.near_zero_rows([x @ B.t() + b]).sum()))
    assert flagged == [1, 0, 0, 2, 13]
