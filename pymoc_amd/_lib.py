"""ctypes binding of libpymoc_hip.so (the C-ABI declared in include/pymoc_hip.h).

The engine has no CPU fallback: if the shared library is missing, importing this module
raises; if no HIP device is visible, the first call that needs one raises.
"""
import ctypes as C
import os

# dmabuf IPC (the only kind this platform's driver supports): RCCL and any cross-process
# sharing of device memory need it, and the HSA runtime reads it when the engine is loaded --
# so it is set here, before the dlopen below, whoever started this process (pymoc_amd.launch,
# torch.distributed.run, a plain shell); an explicit setting by the caller wins
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

_HERE = os.path.dirname(os.path.abspath(__file__))
# PYMOC_HIP_LIB: another build of the same sources (the phase-clock build of profiles/, an A/B
# variant); the product loads the library next to this file
LIB_PATH = os.environ.get("PYMOC_HIP_LIB") or os.path.join(_HERE, "libpymoc_hip.so")

PM_OK, PM_EINVAL, PM_EHIP, PM_ENCCL, PM_ENODEV = 0, 1, 2, 3, 4

PM_COL_DO_CONV, PM_COL_BZBOT, PM_COL_STATIC_IN_RANGE, PM_COL_UNIFORM_AREA = 1, 2, 4, 8
PM_EQ_HFREE, PM_EQ_HAS_BBOT, PM_EQ_KAPPA_ARRAY, PM_EQ_PSI_ARRAY = 1, 2, 4, 8
PM_OP_CONVECT, PM_OP_VERTADVDIFF, PM_OP_HORADV, PM_OP_TIMESTEP, PM_OP_WEFF = 1, 2, 4, 7, 8
PM_OP_CONTRACTED = 16
PM_OP_WA_PSI = 32
PM_OP_WA_TWOBASIN = 64
PM_COLS_ALL_UNIFORM_AREA = 1
PM_COLS_DIV3_PROVEN = 2
PM_COLS_DIV2_GRID = 4
PM_COL_DIV2_AREA = 16

c_dp = C.c_void_p  # device pointers travel as plain addresses


class PmError(RuntimeError):
  def __init__(self, code, text):
    super().__init__("pymoc_hip error %d: %s" % (code, text))
    self.code = code


class pm_columns(C.Structure):
  """Mirror of `struct pm_columns` (include/pymoc_hip.h)."""
  _fields_ = [
      ("ncols", C.c_int32), ("nz", C.c_int32), ("nsel", C.c_int32),
      ("reserved", C.c_int32), ("z", c_dp), ("b", c_dp), ("kappa", c_dp),
      ("area", c_dp), ("dAkappa", c_dp), ("bs", c_dp), ("bbot", c_dp), ("bzbot", c_dp),
      ("N2min", c_dp), ("flags", c_dp), ("ksel", c_dp), ("nonfinite", c_dp),
      ("kappa_base", c_dp), ("kappa_profile", c_dp)
  ]


PM_TW_SOLVE, PM_TW_PSIB, PM_TW_PSIBZ, PM_TW_WA_PSI = 1, 2, 4, 8


class pm_thermwind(C.Structure):
  """Mirror of `struct pm_thermwind` (include/pymoc_hip.h)."""
  _fields_ = [
      ("n", C.c_int32), ("nz", C.c_int32), ("nb", C.c_int32), ("reserved", C.c_int32),
      ("z", c_dp), ("b1", c_dp), ("b2", c_dp), ("f", c_dp), ("Psi", c_dp),
      ("bgrid", c_dp), ("psib", c_dp), ("psibz1", c_dp), ("psibz2", c_dp),
      ("Psi_SO", c_dp), ("wA1", c_dp), ("wA2", c_dp), ("b1_mid", c_dp), ("b2_mid", c_dp),
      ("dPsi", c_dp)
  ]


(PM_SO_HAS_C, PM_SO_BVP_WITH_EK, PM_SO_HAS_HSILL, PM_SO_HAS_HEK, PM_SO_HAS_HTAPERTOP,
 PM_SO_HAS_HTAPERBOT, PM_SO_TAU_ARRAY, PM_SO_NO_FIXUP) = 1, 2, 4, 8, 16, 32, 64, 128
PM_SO_OP_EKMAN, PM_SO_OP_GM, PM_SO_OP_SOLVE = 1, 2, 3
PM_JN_UNIFORM_AREA, PM_JN_CONTRACTED, PM_JN_SHARED_COEF, PM_JN_SPLIT_LANES = 1, 2, 4, 8
PM_JN_DIV3_PROVEN = 16


class pm_psi_so(C.Structure):
  """Mirror of `struct pm_psi_so` (include/pymoc_hip.h)."""
  _fields_ = [
      ("n", C.c_int32), ("nz", C.c_int32), ("ny", C.c_int32), ("flags", C.c_int32),
      ("bvp_refine", C.c_int32), ("reserved", C.c_int32),
      ("z", c_dp), ("y", c_dp), ("b", c_dp), ("bs", c_dp), ("tau", c_dp), ("KGM", c_dp),
      ("f", C.c_double), ("rho", C.c_double), ("L", C.c_double), ("smax", C.c_double),
      ("c", C.c_double), ("Hsill", C.c_double), ("HEk", C.c_double),
      ("Htapertop", C.c_double), ("Htaperbot", C.c_double),
      ("Psi", c_dp), ("Psi_Ek", c_dp), ("Psi_GM", c_dp), ("Ek_raw", c_dp),
      ("GM_raw", c_dp), ("ys", c_dp), ("status", c_dp), ("ys_in", c_dp),
      ("tau_ave_in", c_dp)
  ]


class pm_so_ml(C.Structure):
  """Mirror of `struct pm_so_ml` (include/pymoc_hip.h)."""
  _fields_ = [
      ("n", C.c_int32), ("nz", C.c_int32), ("ny", C.c_int32), ("reserved", C.c_int32),
      ("y", c_dp), ("bs", c_dp), ("Psi_s", c_dp), ("b_basin", c_dp), ("Psi_b", c_dp),
      ("surflux", c_dp), ("rest_mask", c_dp), ("b_rest", c_dp),
      ("Ks", C.c_double), ("h", C.c_double), ("L", C.c_double), ("v_pist", C.c_double),
      ("status", c_dp)
  ]


class pm_column_equi(C.Structure):
  """Mirror of `struct pm_column_equi` (include/pymoc_hip.h)."""
  _fields_ = [
      ("n", C.c_int32), ("nz", C.c_int32), ("mmax", C.c_int32), ("reserved", C.c_int32),
      ("m", c_dp), ("active", c_dp), ("x", c_dp), ("Ak", c_dp), ("dAk", c_dp), ("wA", c_dp),
      ("wA_z", c_dp), ("z", c_dp), ("bs", c_dp), ("bbot", c_dp), ("bzbot", c_dp),
      ("flags", c_dp), ("zidx", c_dp), ("tol", C.c_double), ("y", c_dp), ("rms", c_dp),
      ("nadd", c_dp), ("b", c_dp), ("bz", c_dp)
  ]


class pm_equi_column(C.Structure):
  """Mirror of `struct pm_equi_column` (include/pymoc_hip.h)."""
  _fields_ = [
      ("n", C.c_int32), ("nzg", C.c_int32), ("mmax", C.c_int32), ("reserved", C.c_int32),
      ("m", c_dp), ("active", c_dp), ("x", c_dp), ("y", c_dp), ("yp", c_dp), ("p", c_dp),
      ("f", c_dp), ("A", c_dp), ("bs", c_dp), ("bb", c_dp), ("kappa", c_dp), ("flags", c_dp),
      ("zg", c_dp), ("kappa_z", c_dp), ("dkappa_z", c_dp), ("psi_z", c_dp),
      ("tol", C.c_double), ("rms", c_dp), ("nadd", c_dp), ("status", c_dp), ("niter", c_dp),
      ("info", c_dp), ("scratch", c_dp)
  ]


class pm_jn2018_bc(C.Structure):
  """Mirror of `struct pm_jn2018_bc` (include/pymoc_hip.h)."""
  _fields_ = [
      ("n", C.c_int32), ("nz", C.c_int32), ("ny", C.c_int32), ("reserved", C.c_int32),
      ("Psi_SO", c_dp), ("Psi_res_b", c_dp), ("Psi_res_n", c_dp), ("b_basin", c_dp),
      ("b_north", c_dp), ("bs_SO", c_dp), ("bbot", c_dp), ("ksel", c_dp)
  ]


class pm_jn2018(C.Structure):
  """Mirror of `struct pm_jn2018` (include/pymoc_hip.h)."""
  _fields_ = [
      ("n", C.c_int32), ("hints", C.c_int32), ("reserved1", C.c_int32),
      ("reserved2", C.c_int32), ("cols", pm_columns), ("wA", c_dp), ("Psi_SO", c_dp),
      ("Psi_res_b", c_dp), ("Psi_res_n", c_dp), ("ml", pm_so_ml)
  ]


PM_SEC_CHANNEL, PM_SEC_TWOCOL = 0, 1
PM_SEC_BS_SCALAR, PM_SEC_BN_SCALAR = 1, 2
PM_SEC_FIX_PLOT_OVERTURNING, PM_SEC_FIX_TWOBASIN = 1, 2
PM_SEC_OK, PM_SEC_ESIGN, PM_SEC_ECONV, PM_SEC_ENAN = 0, 1, 2, 3
PM_SEC_MAX_LEVELS = 1024


class pm_sections(C.Structure):
  """Mirror of `struct pm_sections` (include/pymoc_hip.h)."""
  _fields_ = [
      ("n", C.c_int32), ("kind", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32),
      ("nyq", C.c_int32), ("nzq", C.c_int32), ("flags", C.c_int32), ("fixups", C.c_int32),
      ("y", c_dp), ("z", c_dp), ("yq", c_dp), ("zq", c_dp),
      ("bs", c_dp), ("bs_offset", C.c_int64), ("bs_stride", C.c_int64),
      ("bn", c_dp), ("bn_offset", C.c_int64), ("bn_stride", C.c_int64),
      ("out", c_dp), ("status", c_dp), ("first", c_dp)
  ]


PM_OVT_Z, PM_OVT_B, PM_OVT_RES = 0, 1, 2
PM_OVT_NAN_SECTION, PM_OVT_BAD_BASIN = 1, 2
PM_OVT_MAX_LEVELS, PM_OVT_MAX_NB = 1024, 2048


class pm_rows(C.Structure):
  """Mirror of `struct pm_rows` (include/pymoc_hip.h)."""
  _fields_ = [("ptr", c_dp), ("offset", C.c_int64), ("stride", C.c_int64)]


class pm_overturning(C.Structure):
  """Mirror of `struct pm_overturning` (include/pymoc_hip.h)."""
  _fields_ = [
      ("n", C.c_int32), ("nz", C.c_int32), ("ny", C.c_int32), ("nb", C.c_int32),
      ("n_basin", C.c_int32), ("n_north", C.c_int32), ("reserved1", C.c_int32),
      ("reserved2", C.c_int32),
      ("b_basin", pm_rows), ("bs_SO", pm_rows), ("Psi", pm_rows), ("Psi_SO", pm_rows),
      ("bgrid", pm_rows), ("psib", pm_rows), ("psibz1", pm_rows), ("bsouth", pm_rows),
      ("bnorth", pm_rows), ("c1", c_dp), ("c2", c_dp), ("c3", c_dp),
      ("lbasin", C.c_double), ("lnorth", C.c_double),
      ("psi_z", c_dp), ("psi_b", c_dp), ("psi_res", c_dp), ("bnew", c_dp),
      ("extrema", c_dp), ("extrema_at", c_dp), ("status", c_dp)
  ]


PM_TBO_FIELDS = 8
(PM_TBO_NAN_SECTION, PM_TBO_BAD_BASIN, PM_TBO_BAD_ATL, PM_TBO_BAD_PAC, PM_TBO_BAD_BGRID_AMOC,
 PM_TBO_BAD_BGRID_ZOC) = 1, 2, 4, 8, 16, 32
PM_TBO_MAX_LEVELS, PM_TBO_MAX_NB = 1024, 2048
LDS_PER_CU = 160 * 1024


class pm_twobasin_rows(C.Structure):
  """Mirror of `struct pm_twobasin_rows` (include/pymoc_hip.h)."""
  _fields_ = [("n", C.c_int32), ("nz", C.c_int32), ("b_Atl", pm_rows), ("b_Pac", pm_rows),
              ("b_north", pm_rows), ("A_Atl", pm_rows), ("A_Pac", pm_rows), ("b_basin", c_dp),
              ("bn", c_dp)]


class pm_twobasin_overturning(C.Structure):
  """Mirror of `struct pm_twobasin_overturning` (include/pymoc_hip.h)."""
  ROWS = ("b_Atl", "b_Pac", "A_Atl", "A_Pac", "bs_SO", "Psi_SO_Atl", "Psi_SO_Pac", "Psi_AMOC",
          "Psi_ZOC", "psibz_AMOC1", "psibz_AMOC2", "psibz_ZOC1", "psibz_ZOC2", "bgrid_AMOC",
          "psib_AMOC", "bgrid_ZOC", "psib_ZOC", "bsouth", "btrans", "bn")
  _fields_ = [
      ("n", C.c_int32), ("nz", C.c_int32), ("ny", C.c_int32), ("nb", C.c_int32),
      ("n_basin", C.c_int32), ("n_trans", C.c_int32), ("n_north", C.c_int32),
      ("reserved", C.c_int32)] + [(r, pm_rows) for r in ROWS] + [
      ("c1", c_dp), ("c2", c_dp), ("c3", c_dp), ("lbasin", C.c_double), ("lnorth", C.c_double),
      ("psi", c_dp * PM_TBO_FIELDS), ("bnew", c_dp), ("bnew_Atl", c_dp), ("bnew_Pac", c_dp),
      ("extrema", c_dp), ("extrema_at", c_dp), ("status", c_dp)
  ]


PM_PACK_MAX_ITEMS = 8


class pm_row_copy(C.Structure):
  """Mirror of `struct pm_row_copy` (include/pymoc_hip.h)."""
  _fields_ = [("src", c_dp), ("dst", c_dp), ("nlev", C.c_int32), ("src_stride", C.c_int32)]


class pm_run_schedule(C.Structure):
  """Mirror of `struct pm_run_schedule` (include/pymoc_hip.h)."""
  _fields_ = [("n_first", C.c_int32), ("n_updates", C.c_int32), ("m_steps", C.c_int32),
              ("n_last", C.c_int32)]


class pm_twocol_loop(C.Structure):
  """Mirror of `struct pm_twocol_loop` (include/pymoc_hip.h)."""
  _fields_ = [("cols", pm_columns), ("tw", pm_thermwind), ("wA", c_dp), ("dt", C.c_double),
              ("sched", pm_run_schedule), ("status", c_dp)]


class pm_jn2018_loop(C.Structure):
  """Mirror of `struct pm_jn2018_loop` (include/pymoc_hip.h)."""
  _fields_ = [("jn", pm_jn2018), ("tw", pm_thermwind), ("so", pm_psi_so), ("dt", C.c_double),
              ("sched", pm_run_schedule)]


PM_STEADY_RUNNING, PM_STEADY_CONVERGED, PM_STEADY_NONFINITE, PM_STEADY_MAXSTEPS = 0, 1, 2, 3
PM_STEADY_MAX_DRIFT, PM_STEADY_MAX_CAPTURE = 4, 8


class pm_steady_field(C.Structure):
  """Mirror of `struct pm_steady_field` (include/pymoc_hip.h)."""
  _fields_ = [("src", c_dp), ("src_stride", C.c_int64), ("buf", c_dp), ("len", C.c_int32),
              ("reserved", C.c_int32)]


class pm_steady_check(C.Structure):
  """Mirror of `struct pm_steady_check` (include/pymoc_hip.h)."""
  _fields_ = [
      ("n", C.c_int32), ("n0", C.c_int32), ("ndrift", C.c_int32), ("ncapture", C.c_int32),
      ("consecutive", C.c_int32), ("finalize", C.c_int32), ("step", C.c_int64),
      ("scale", C.c_double), ("orig", c_dp), ("tol", c_dp), ("streak", c_dp), ("status", c_dp),
      ("drift_out", c_dp), ("step_out", c_dp), ("n_running", c_dp),
      ("drift", pm_steady_field * PM_STEADY_MAX_DRIFT),
      ("capture", pm_steady_field * PM_STEADY_MAX_CAPTURE)
  ]


PM_FORCING_MAX_TARGETS = 8


class pm_forcing_target(C.Structure):
  """Mirror of `struct pm_forcing_target` (include/pymoc_hip.h)."""
  _fields_ = [("dst", c_dp), ("row0", C.c_int64), ("values", c_dp), ("len", C.c_int32),
              ("per_member", C.c_int32)]


class pm_forcing(C.Structure):
  """Mirror of `struct pm_forcing` (include/pymoc_hip.h); `knots` is a HOST address."""
  _fields_ = [("n", C.c_int32), ("K", C.c_int32), ("ntargets", C.c_int32),
              ("reserved", C.c_int32), ("knots", C.c_void_p),
              ("target", pm_forcing_target * PM_FORCING_MAX_TARGETS)]


PM_NOISE_MAX_TARGETS, PM_NOISE_STREAMS = 8, 6


class pm_noise_target(C.Structure):
  """Mirror of `struct pm_noise_target` (include/pymoc_hip.h)."""
  _fields_ = [("dst", c_dp), ("row0", C.c_int64), ("base", c_dp), ("pattern", c_dp),
              ("sigma", c_dp), ("x_in", c_dp), ("x_out", c_dp), ("xi_out", c_dp),
              ("a", C.c_double), ("b", C.c_double), ("len", C.c_int32),
              ("pattern_per_member", C.c_int32), ("stream", C.c_int32), ("reserved", C.c_int32)]


class pm_noise(C.Structure):
  """Mirror of `struct pm_noise` (include/pymoc_hip.h)."""
  _fields_ = [("n", C.c_int32), ("ntargets", C.c_int32), ("j", C.c_uint32),
              ("reserved", C.c_uint32), ("seed", C.c_uint64), ("member0", C.c_int64),
              ("target", pm_noise_target * PM_NOISE_MAX_TARGETS)]


PM_INDICES_MAX = 32
PM_IDX_MAX, PM_IDX_MIN, PM_IDX_AT, PM_IDX_CROSS, PM_IDX_MEAN = 0, 1, 2, 3, 4


class pm_index_spec(C.Structure):
  """Mirror of `struct pm_index_spec` (include/pymoc_hip.h)."""
  _fields_ = [("src", c_dp), ("axis", c_dp), ("stride", C.c_int64), ("nlev", C.c_int32),
              ("kind", C.c_int32), ("lo", C.c_int32), ("hi", C.c_int32), ("param", C.c_double)]


class pm_row_indices(C.Structure):
  """Mirror of `struct pm_row_indices` (include/pymoc_hip.h); `spec` is a HOST address."""
  _fields_ = [("n", C.c_int32), ("nspec", C.c_int32), ("spec", C.c_void_p), ("spec_dev", c_dp)]


PM_STATS_Q_MAX, PM_STATS_LAG_MAX, PM_STATS_GROUP_MAX, PM_STATS_CHUNK = 8, 4, 8192, 256


class pm_series_group_stats(C.Structure):
  """Mirror of `struct pm_series_group_stats` (include/pymoc_hip.h); `start` and `q` are HOST
  addresses."""
  _fields_ = [("n", C.c_int32), ("nspec", C.c_int32), ("nrec", C.c_int32), ("k0", C.c_int32),
              ("k1", C.c_int32), ("ngroups", C.c_int32), ("nq", C.c_int32),
              ("reserved", C.c_int32), ("v", c_dp), ("order", c_dp), ("start", C.c_void_p),
              ("start_dev", c_dp), ("q", C.c_void_p), ("q_dev", c_dp)]


class pm_series_member_stats(C.Structure):
  """Mirror of `struct pm_series_member_stats` (include/pymoc_hip.h); `lag`, `thr` and `dir` are
  HOST addresses."""
  _fields_ = [("n", C.c_int32), ("nspec", C.c_int32), ("nrec", C.c_int32), ("k0", C.c_int32),
              ("k1", C.c_int32), ("nlag", C.c_int32), ("reserved1", C.c_int32),
              ("reserved2", C.c_int32), ("v", c_dp), ("lag", C.c_void_p), ("lag_dev", c_dp),
              ("thr", C.c_void_p), ("thr_dev", c_dp), ("dir", C.c_void_p), ("dir_dev", c_dp)]


PM_SPEC_NPERSEG_MIN, PM_SPEC_NPERSEG_MAX, PM_SPEC_PAIRS_MAX = 8, 1024, 8
PM_SPEC_DETREND_NONE, PM_SPEC_DETREND_CONSTANT = 0, 1


class pm_series_spectra(C.Structure):
  """Mirror of `struct pm_series_spectra` (include/pymoc_hip.h); `window` and `pair` are HOST
  addresses."""
  _fields_ = [("n", C.c_int32), ("nspec", C.c_int32), ("nrec", C.c_int32), ("k0", C.c_int32),
              ("k1", C.c_int32), ("nperseg", C.c_int32), ("step", C.c_int32),
              ("detrend", C.c_int32), ("npairs", C.c_int32), ("reserved", C.c_int32),
              ("v", c_dp), ("window", C.c_void_p), ("window_dev", c_dp), ("twiddle", c_dp),
              ("pair", C.c_void_p), ("pair_dev", c_dp), ("scale", C.c_double)]


PM_WIN_MIN, PM_WIN_MAX, PM_KENDALL_MAX = 4, 4096, 4096
PM_WIN_DETREND_NONE, PM_WIN_DETREND_CONSTANT, PM_WIN_DETREND_LINEAR = 0, 1, 2


class pm_series_windows(C.Structure):
  """Mirror of `struct pm_series_windows` (include/pymoc_hip.h)."""
  _fields_ = [("n", C.c_int32), ("nspec", C.c_int32), ("nrec", C.c_int32), ("k0", C.c_int32),
              ("k1", C.c_int32), ("window", C.c_int32), ("step", C.c_int32), ("lag", C.c_int32),
              ("detrend", C.c_int32), ("reserved", C.c_int32), ("v", c_dp), ("stt", C.c_double)]


PM_DFA_SCALES_MAX, PM_DFA_SCALE_MIN = 16, 4


class pm_series_dfa(C.Structure):
  """Mirror of `struct pm_series_dfa` (include/pymoc_hip.h)."""
  _fields_ = [("n", C.c_int32), ("nspec", C.c_int32), ("nrec", C.c_int32), ("k0", C.c_int32),
              ("k1", C.c_int32), ("window", C.c_int32), ("step", C.c_int32),
              ("detrend", C.c_int32), ("nq", C.c_int32), ("reserved", C.c_int32), ("v", c_dp),
              ("stt", C.c_double), ("scale", C.c_int32 * PM_DFA_SCALES_MAX),
              ("suu", C.c_double * PM_DFA_SCALES_MAX), ("weight", C.c_double * PM_DFA_SCALES_MAX)]


PM_RESTORE_WIN_MIN, PM_RESTORE_ITERS_MAX = 8, 64


class pm_series_restoring(C.Structure):
  """Mirror of `struct pm_series_restoring` (include/pymoc_hip.h)."""
  _fields_ = [("n", C.c_int32), ("nspec", C.c_int32), ("nrec", C.c_int32), ("k0", C.c_int32),
              ("k1", C.c_int32), ("window", C.c_int32), ("step", C.c_int32),
              ("detrend", C.c_int32), ("iters", C.c_int32), ("reserved", C.c_int32), ("v", c_dp),
              ("stt", C.c_double)]


PM_EOF_Q_MAX, PM_EOF_ITERS_MAX = 32, 1024


class pm_series_scatter(C.Structure):
  """Mirror of `struct pm_series_scatter` (include/pymoc_hip.h)."""
  _fields_ = [("n", C.c_int32), ("nspec", C.c_int32), ("nrec", C.c_int32), ("k0", C.c_int32),
              ("k1", C.c_int32), ("q", C.c_int32), ("reserved1", C.c_int32),
              ("reserved2", C.c_int32), ("v", c_dp), ("w", c_dp),
              ("sel", C.c_int32 * PM_EOF_Q_MAX)]


class pm_series_eof(C.Structure):
  """Mirror of `struct pm_series_eof` (include/pymoc_hip.h); `start` is a HOST address."""
  _fields_ = [("n", C.c_int32), ("q", C.c_int32), ("nu", C.c_int32), ("iters", C.c_int32),
              ("nused", c_dp), ("scat", c_dp), ("order", c_dp), ("start", C.c_void_p),
              ("start_dev", c_dp)]


class pm_series_project(C.Structure):
  """Mirror of `struct pm_series_project` (include/pymoc_hip.h)."""
  _fields_ = [("n", C.c_int32), ("nspec", C.c_int32), ("nrec", C.c_int32), ("k0", C.c_int32),
              ("k1", C.c_int32), ("q", C.c_int32), ("nu", C.c_int32), ("reserved", C.c_int32),
              ("v", c_dp), ("w", c_dp), ("nused", c_dp), ("mean", c_dp), ("eof", c_dp),
              ("unit", c_dp), ("sel", C.c_int32 * PM_EOF_Q_MAX)]


class pm_series_kendall(C.Structure):
  """Mirror of `struct pm_series_kendall` (include/pymoc_hip.h)."""
  _fields_ = [("n", C.c_int32), ("nspec", C.c_int32), ("nrec", C.c_int32), ("k0", C.c_int32),
              ("k1", C.c_int32), ("reserved1", C.c_int32), ("reserved2", C.c_int32),
              ("reserved3", C.c_int32), ("v", c_dp)]


PM_SURROGATE_MAX = 4096


class pm_series_surrogates(C.Structure):
  """Mirror of `struct pm_series_surrogates` (include/pymoc_hip.h)."""
  _fields_ = [("n", C.c_int32), ("nspec", C.c_int32), ("K", C.c_int32), ("nb", C.c_int32),
              ("b0", C.c_int64), ("member0", C.c_int64), ("seed", C.c_uint64), ("var", c_dp),
              ("ac", c_dp)]


class pm_series_exceed(C.Structure):
  """Mirror of `struct pm_series_exceed` (include/pymoc_hip.h)."""
  _fields_ = [("n", C.c_int32), ("nspec", C.c_int32), ("nb", C.c_int32), ("reserved", C.c_int32),
              ("obs_conc", c_dp), ("obs_disc", c_dp), ("obs_tie", c_dp), ("sur_conc", c_dp),
              ("sur_disc", c_dp), ("sur_tie", c_dp)]


PM_SMOOTH_MAX, PM_SMOOTH_HALF_MAX = 4096, 4095


class pm_series_smooth(C.Structure):
  """Mirror of `struct pm_series_smooth` (include/pymoc_hip.h); `w` is a HOST address."""
  _fields_ = [("n", C.c_int32), ("nspec", C.c_int32), ("nrec", C.c_int32), ("k0", C.c_int32),
              ("k1", C.c_int32), ("half", C.c_int32), ("reserved1", C.c_int32),
              ("reserved2", C.c_int32), ("v", c_dp), ("w", C.c_void_p), ("w_dev", c_dp)]


PM_SHIFT_HALF_MAX = 2048


class pm_series_shift_scan(C.Structure):
  """Mirror of `struct pm_series_shift_scan` (include/pymoc_hip.h); `thr` and `dir` are HOST
  addresses."""
  _fields_ = [("n", C.c_int32), ("nspec", C.c_int32), ("nrec", C.c_int32), ("k0", C.c_int32),
              ("k1", C.c_int32), ("half", C.c_int32), ("reserved1", C.c_int32),
              ("reserved2", C.c_int32), ("mean", c_dp), ("var", c_dp), ("thr", C.c_void_p),
              ("thr_dev", c_dp), ("dir", C.c_void_p), ("dir_dev", c_dp)]


class pm_series_censor(C.Structure):
  """Mirror of `struct pm_series_censor` (include/pymoc_hip.h); `src` is a HOST address."""
  _fields_ = [("n", C.c_int32), ("nspec", C.c_int32), ("K", C.c_int32), ("nb", C.c_int32),
              ("guard", C.c_int32), ("reserved", C.c_int32), ("x", c_dp), ("where", c_dp),
              ("src", C.c_void_p), ("src_dev", c_dp)]


class pm_series_fit_ranged(C.Structure):
  """Mirror of `struct pm_series_fit_ranged` (include/pymoc_hip.h); `stt_tab` is a HOST address."""
  _fields_ = [("n", C.c_int32), ("nspec", C.c_int32), ("nrec", C.c_int32), ("k0", C.c_int32),
              ("k1", C.c_int32), ("detrend", C.c_int32), ("reserved1", C.c_int32),
              ("reserved2", C.c_int32), ("v", c_dp), ("end", c_dp), ("stt_tab", C.c_void_p),
              ("stt_tab_dev", c_dp)]


class pm_series_fourier_coef(C.Structure):
  """Mirror of `struct pm_series_fourier_coef` (include/pymoc_hip.h); `tw`, `chirp` and `filt` are
  HOST addresses."""
  _fields_ = [("n", C.c_int32), ("nspec", C.c_int32), ("nrec", C.c_int32), ("k0", C.c_int32),
              ("k1", C.c_int32), ("detrend", C.c_int32), ("M", C.c_int32), ("reserved", C.c_int32),
              ("v", c_dp), ("stt", C.c_double), ("tw", C.c_void_p), ("chirp", C.c_void_p),
              ("filt", C.c_void_p), ("tw_dev", c_dp), ("chirp_dev", c_dp), ("filt_dev", c_dp)]


class pm_series_surrogates_fourier(C.Structure):
  """Mirror of `struct pm_series_surrogates_fourier` (include/pymoc_hip.h); `tw`, `chirp`, `filt`,
  `ph_hi` and `ph_lo` are HOST addresses."""
  _fields_ = [("n", C.c_int32), ("nspec", C.c_int32), ("K", C.c_int32), ("nb", C.c_int32),
              ("b0", C.c_int64), ("member0", C.c_int64), ("seed", C.c_uint64), ("M", C.c_int32),
              ("reserved", C.c_int32), ("coef", c_dp), ("tw", C.c_void_p), ("chirp", C.c_void_p),
              ("filt", C.c_void_p), ("ph_hi", C.c_void_p), ("ph_lo", C.c_void_p), ("tw_dev", c_dp),
              ("chirp_dev", c_dp), ("filt_dev", c_dp), ("ph_hi_dev", c_dp), ("ph_lo_dev", c_dp),
              ("scratch", c_dp)]


if not os.path.exists(LIB_PATH):
  raise ImportError(
      "pymoc_amd: %s is missing. Build it with `make lib` (hipcc --offload-arch=gfx950) "
      "or `python -c 'import __graft_entry__ as g; g.build()'`. There is no CPU "
      "fallback." % LIB_PATH)

lib = C.CDLL(LIB_PATH)

# name -> (restype, argtypes); every symbol include/pymoc_hip.h declares
SIGNATURES = {
    "pm_version": (C.c_char_p, []),
    "pm_last_error": (C.c_char_p, []),
    "pm_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "pm_set_device": (C.c_int, [C.c_int]),
    "pm_device_info": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_int),
                                 C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "pm_malloc": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t]),
    "pm_free": (C.c_int, [C.c_void_p]),
    "pm_memset": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]),
    "pm_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pm_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pm_memcpy_d2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pm_host_alloc": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t]),
    "pm_host_free": (C.c_int, [C.c_void_p]),
    "pm_memcpy_d2h_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pm_rows_pack": (C.c_int, [C.c_void_p, C.c_int32, c_dp, C.c_int32, C.c_void_p]),
    "pm_stream_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "pm_stream_create_priority": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "pm_stream_destroy": (C.c_int, [C.c_void_p]),
    "pm_stream_sync": (C.c_int, [C.c_void_p]),
    "pm_device_sync": (C.c_int, []),
    "pm_event_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "pm_event_destroy": (C.c_int, [C.c_void_p]),
    "pm_event_record": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pm_event_sync": (C.c_int, [C.c_void_p]),
    "pm_stream_wait_event": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pm_twocol_forcing": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "pm_event_elapsed_ms": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]),
    "pm_graph_begin_capture": (C.c_int, [C.c_void_p]),
    "pm_graph_end_capture": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "pm_graph_launch": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pm_graph_destroy": (C.c_int, [C.c_void_p]),
    "pm_column_steps": (C.c_int, [C.POINTER(pm_columns), c_dp, c_dp, c_dp, C.c_double,
                                  C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "pm_column_steps_implicit": (C.c_int, [C.POINTER(pm_columns), c_dp, C.c_double, C.c_int32,
                                           C.c_int32, C.c_void_p]),
    "pm_column_steps_implicit_twobasin": (C.c_int, [C.POINTER(pm_columns), c_dp, c_dp, c_dp,
                                                    C.c_double, C.c_int32, C.c_int32, C.c_void_p]),
    "pm_column_weff": (C.c_int, [C.POINTER(pm_columns), c_dp, c_dp, C.c_void_p]),
    "pm_column_kernel_shape": (C.c_int, [C.c_int32, C.c_int32, C.c_int32,
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "pm_column_kernel_name": (C.c_int, [C.POINTER(pm_columns), c_dp, c_dp, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_char_p, C.c_size_t]),
    "pm_column_kernel_twin": (C.c_int, [C.POINTER(pm_columns), c_dp, c_dp, C.c_int32, C.c_int32,
                                        C.c_int32, C.POINTER(C.c_int32)]),
    "pm_thermwind_update": (C.c_int, [C.POINTER(pm_thermwind), C.c_int32, C.c_void_p]),
    "pm_thermwind_residuals": (C.c_int, [C.c_int32] + [c_dp] * 6 + [C.c_void_p]),
    "pm_psi_so_update": (C.c_int, [C.POINTER(pm_psi_so), C.c_int32, C.c_void_p]),
    "pm_so_ml_step": (C.c_int, [C.POINTER(pm_so_ml), C.c_double, C.c_void_p]),
    "pm_jn2018_bc_switch": (C.c_int, [C.POINTER(pm_jn2018_bc), C.c_void_p]),
    "pm_jn2018_steps": (C.c_int, [C.POINTER(pm_jn2018), C.c_double, C.c_int32, C.c_void_p]),
    "pm_jn2018_steps_implicit": (C.c_int, [C.POINTER(pm_jn2018), C.c_double, C.c_int32,
                                           C.c_void_p]),
    "pm_twocol_run": (C.c_int, [C.POINTER(pm_twocol_loop), C.c_void_p]),
    "pm_jn2018_run": (C.c_int, [C.POINTER(pm_jn2018_loop), C.c_void_p]),
    "pm_so_tw_update": (C.c_int, [C.POINTER(pm_psi_so), C.POINTER(pm_thermwind), C.c_int32,
                                  C.c_void_p]),
    "pm_run_lds_bytes": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                   C.POINTER(C.c_size_t)]),
    "pm_twobasin_forcing": (C.c_int, [C.c_int32, C.c_int32] + [c_dp] * 9 + [C.c_void_p]),
    "pm_column_equi_pass": (C.c_int, [C.POINTER(pm_column_equi), C.c_void_p]),
    "pm_equi_column_scratch_doubles": (C.c_size_t, [C.c_int32]),
    "pm_equi_column_newton": (C.c_int, [C.POINTER(pm_equi_column), C.c_void_p]),
    "pm_axpby": (C.c_int, [C.c_size_t, C.c_double, c_dp, C.c_double, c_dp, c_dp, C.c_void_p]),
    "pm_comm_unique_id": (C.c_int, [C.c_void_p]),
    "pm_comm_init": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_void_p]),
    "pm_comm_destroy": (C.c_int, [C.c_void_p]),
    "pm_comm_allgather": (C.c_int, [C.c_void_p, c_dp, c_dp, C.c_size_t, C.c_void_p]),
    "pm_comm_gather_root": (C.c_int, [C.c_void_p, c_dp, c_dp, C.c_size_t, C.c_int32, C.c_int32,
                                      C.c_void_p]),
    "pm_comm_allreduce_max": (C.c_int, [C.c_void_p, c_dp, c_dp, C.c_size_t, C.c_void_p]),
    "pm_comm_barrier": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pm_selftest_fastdiv": (C.c_int, [C.c_uint64, C.c_int32, C.c_int32, C.c_int32,
                                      C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "pm_selftest_lane_shift": (C.c_int, [C.POINTER(C.c_int32)]),
    "pm_div3_proven": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "pm_recip_check": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]),
    "pm_div2_proven": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int64)]),
    "pm_recip2_check": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "pm_selftest_div2": (C.c_int, [C.c_uint64, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "pm_selftest_div3": (C.c_int, [C.c_uint64, C.c_int32, C.POINTER(C.c_uint64),
                                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                   C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "pm_selftest_so_scans": (C.c_int, [C.c_int32, C.c_uint64, C.POINTER(C.c_double),
                                       C.POINTER(C.c_int32)]),
    "pm_sections_grid": (C.c_int, [C.POINTER(pm_sections), C.c_void_p]),
    "pm_overturning_sections": (C.c_int, [C.POINTER(pm_overturning), C.c_void_p]),
    "pm_twobasin_profiles": (C.c_int, [C.POINTER(pm_twobasin_rows), C.c_void_p]),
    "pm_twobasin_overturning_lds_bytes": (C.c_int, [C.c_int32, C.c_int32, C.c_int32,
                                                    C.POINTER(C.c_size_t)]),
    "pm_twobasin_overturning_sections": (C.c_int, [C.POINTER(pm_twobasin_overturning),
                                                   C.c_void_p]),
    "pm_steady_check": (C.c_int, [C.POINTER(pm_steady_check), C.c_void_p]),
    "pm_forcing_apply": (C.c_int, [C.POINTER(pm_forcing), C.c_double, C.c_void_p]),
    "pm_row_indices": (C.c_int, [C.POINTER(pm_row_indices), c_dp, c_dp, C.c_void_p]),
    "pm_forcing_noise": (C.c_int, [C.POINTER(pm_noise), C.c_void_p]),
    "pm_series_group_stats": (C.c_int, [C.POINTER(pm_series_group_stats), c_dp, c_dp, C.c_void_p]),
    "pm_series_member_stats": (C.c_int, [C.POINTER(pm_series_member_stats), c_dp, c_dp, c_dp, c_dp,
                                         C.c_void_p]),
    "pm_series_spectra": (C.c_int, [C.POINTER(pm_series_spectra), c_dp, c_dp, c_dp, c_dp,
                                    C.c_void_p]),
    "pm_series_windows": (C.c_int, [C.POINTER(pm_series_windows), c_dp, c_dp, C.c_void_p]),
    "pm_series_windows_geometry": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                             C.POINTER(C.c_int32)]),
    "pm_series_kendall": (C.c_int, [C.POINTER(pm_series_kendall), c_dp, c_dp, c_dp, c_dp,
                                    C.c_void_p]),
    "pm_series_dfa": (C.c_int, [C.POINTER(pm_series_dfa), c_dp, c_dp, C.c_void_p]),
    "pm_series_restoring": (C.c_int, [C.POINTER(pm_series_restoring), c_dp, c_dp, C.c_void_p]),
    "pm_series_scatter": (C.c_int, [C.POINTER(pm_series_scatter), c_dp, c_dp, c_dp, C.c_void_p]),
    "pm_series_eof": (C.c_int, [C.POINTER(pm_series_eof)] + [c_dp] * 6 + [C.c_void_p]),
    "pm_series_project": (C.c_int, [C.POINTER(pm_series_project), c_dp, C.c_void_p]),
    "pm_series_surrogates": (C.c_int, [C.POINTER(pm_series_surrogates), c_dp, c_dp, C.c_void_p]),
    "pm_series_exceed": (C.c_int, [C.POINTER(pm_series_exceed), c_dp, c_dp, c_dp, C.c_void_p]),
    "pm_series_smooth": (C.c_int, [C.POINTER(pm_series_smooth), c_dp, c_dp, c_dp, C.c_void_p]),
    "pm_series_smooth_geometry": (C.c_int, [C.c_int32, C.POINTER(C.c_int32),
                                            C.POINTER(C.c_int32)]),
    "pm_series_smooth_lds_bytes": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "pm_series_shift_scan": (C.c_int, [C.POINTER(pm_series_shift_scan), c_dp, c_dp, c_dp, c_dp,
                                       C.c_void_p]),
    "pm_series_censor": (C.c_int, [C.POINTER(pm_series_censor), c_dp, c_dp, C.c_void_p]),
    "pm_series_fit_ranged": (C.c_int, [C.POINTER(pm_series_fit_ranged), c_dp, c_dp, C.c_void_p]),
    "pm_series_fourier_coef": (C.c_int, [C.POINTER(pm_series_fourier_coef), c_dp, C.c_void_p]),
    "pm_series_surrogates_fourier": (C.c_int, [C.POINTER(pm_series_surrogates_fourier), c_dp,
                                               C.c_void_p]),
}

for _name, (_res, _args) in SIGNATURES.items():
  _fn = getattr(lib, _name)  # AttributeError here = header/library mismatch
  _fn.restype = _res
  _fn.argtypes = _args


def check(rc):
  if rc != PM_OK:
    raise PmError(rc, lib.pm_last_error().decode("utf-8", "replace"))


_device_ready = False


def require_device(device=None):
  """Select the HIP device once; raises PmError(PM_ENODEV) when none is visible."""
  global _device_ready
  if _device_ready and device is None:
    return
  n = C.c_int(0)
  check(lib.pm_device_count(C.byref(n)))
  if n.value <= 0:
    raise PmError(PM_ENODEV, "no HIP device visible; pymoc_amd has no CPU fallback")
  if device is None:
    device = int(os.environ.get("LOCAL_RANK", "0")) % n.value
  check(lib.pm_set_device(int(device)))
  _device_ready = True


def device_info():
  require_device()
  name = C.create_string_buffer(256)
  cus, mem, clk = C.c_int(0), C.c_size_t(0), C.c_int(0)
  check(lib.pm_device_info(name, 256, C.byref(cus), C.byref(mem), C.byref(clk)))
  return {"name": name.value.decode(), "compute_units": cus.value,
          "hbm_bytes": mem.value, "clock_mhz": clk.value}
