"""pymoc_amd/series.py: SeriesStats, SeriesSpectra and SeriesWindows take a source and a record
window through one piece of code, so a bad one is refused by all three with the same words, on the
host, before any device call."""
import numpy as np
import pytest


class _Series(object):
  """A stand-in for a device series: a shape and a dtype, no memory."""

  def __init__(self, shape, dtype=np.float64):
    self.shape, self.dtype, self.ptr = shape, np.dtype(dtype), 0


class _Recorder(object):
  """A stand-in for an IndexRecorder of 40 records, the last four never written."""

  class _T(object):
    names = ["wind", "amoc"]

  class _E(object):
    stream = timer = None

  def __init__(self):
    self._values, self.table, self.ens = _Series((40, 2, 6)), self._T(), self._E()
    self.steps = np.where(np.arange(40) < 36, np.arange(40) * 12, -1)


def _stats(source):
  from pymoc_amd import SeriesStats
  return SeriesStats(source).across_members


def _spectra(source):
  from pymoc_amd import SeriesSpectra
  return SeriesSpectra(source, 8).compute


def _windows(source):
  from pymoc_amd import SeriesWindows
  return SeriesWindows(source, 8).compute


SHAPE = "the series must be a float64 device array [nrec, nspec, n] (shape %s here)"
TUPLE = "a source is an IndexRecorder or (DeviceArray [nrec, nspec, n], names)"
NAMES = "the series has 2 indices but %d distinct names are given"
BAD_SOURCES = [
    ((_Series((10, 2)), ["a", "b"]), SHAPE % "(10, 2)"),
    ((_Series((10, 2, 6), np.float32), ["a", "b"]), SHAPE % "(10, 2, 6)"),
    ((_Series((10, 0, 6)), []), SHAPE % "(10, 0, 6)"),
    ((np.zeros(3), ["a", "b"]), SHAPE % "(3,)"),
    ((None, ["a", "b"]), SHAPE % "()"),
    ((_Series((10, 2, 6)),), TUPLE),
    ((_Series((10, 2, 6)), ["a", "b"], None), TUPLE),
    ((_Series((10, 2, 6)), ["amoc"]), NAMES % 1),
    ((_Series((10, 2, 6)), ["amoc", "amoc"]), NAMES % 1),
    ((_Series((10, 2, 6)), ["a", "b", "c"]), NAMES % 3),
]
OUTSIDE = "window [%d, %d) is not inside the 40 records"
UNWRITTEN = "window [%d, %d) holds record 36, which was never written"
# (k0, k1) on the recorder; [34, 38) is also shorter than nperseg and than the window length, 8:
# the shared check comes first
BAD_WINDOWS = [
    ((-1, 20), OUTSIDE % (-1, 20)),
    ((20, 20), OUTSIDE % (20, 20)),
    ((30, 10), OUTSIDE % (30, 10)),
    ((0, 41), OUTSIDE % (0, 41)),
    ((40, None), OUTSIDE % (40, 40)),
    ((), UNWRITTEN % (0, 40)),
    ((20, 37), UNWRITTEN % (20, 37)),
    ((34, 38), UNWRITTEN % (34, 38)),
]


@pytest.mark.parametrize("make", [_stats, _spectra, _windows])
def test_every_series_class_refuses_in_the_same_words(make):
  for source, text in BAD_SOURCES:
    with pytest.raises(ValueError) as e:
      make(source)
    assert str(e.value) == text, source
  for source in (_Recorder(), (_Series((40, 2, 6)), ["wind", "amoc"])):
    call = make(source)
    for window, text in BAD_WINDOWS:
      if "never written" in text and isinstance(source, tuple):
        continue  # (a plain series has no record of what was written)
      with pytest.raises(ValueError) as e:
        call(*window)
      assert str(e.value) == text, window
