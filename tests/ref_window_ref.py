"""numpy restatement of the reference window of a path-following MPC step (include/cddp_hip.h, cddp_hip_mpc_set_reference_path;
cddp-cpp_amd/csrc/ref_window.hpp), for tests/test_ref_window_host.py (which holds it to the header's function, bit for bit) and the GPU
tests of the bound path.  Nothing here is imported by the product, and nothing here touches a device.

  window row t of cursor k (t = 0 .. N), path rows p_0 .. p_{L-1}:
      pos = float(k + t) * rows_per_step;  i = floor(pos);  a = pos - i
      row t = p_{L-1}                          when i >= L - 1
      row t = p_i + a * (p_{i+1} - p_i)        otherwise  (one rounding per operation, as the library without FMA contraction)
  goal = row N."""
import math

import numpy as np


def window(path, k, N, rows_per_step=1.0):
    """-> (N + 1, nx) float64"""
    path = np.asarray(path, dtype=np.float64)
    L, nx = path.shape
    out = np.empty((N + 1, nx))
    for t in range(N + 1):
        pos = float(k + t) * float(rows_per_step)
        i = math.floor(pos) if math.isfinite(pos) else L
        if i >= L - 1:
            out[t] = path[L - 1]
        else:
            a = np.float64(pos - float(i))
            out[t] = path[i] + a * (path[i + 1] - path[i])
    return out


def goal(path, k, N, rows_per_step=1.0):
    return window(path, k, N, rows_per_step)[N].copy()
