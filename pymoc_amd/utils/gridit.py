"""`pymoc.utils.gridit` (src/pymoc/utils/gridit.py:4-30): a[i, j] = f(x1[i], x2[j]), filled in
row-major order; the first exception f raises propagates.  The section interpolators of
pymoc_amd.plotting have their own `gridit` method, which fills the whole grid in one launch."""
import numpy as np


def gridit(x1, x2, f):
  n1 = len(x1)
  n2 = len(x2)
  array = np.zeros((n1, n2))
  for i in range(0, n1):
    for j in range(0, n2):
      array[i, j] = f(x1[i], x2[j])
  return array
