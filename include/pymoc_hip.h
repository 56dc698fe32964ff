/*
 * pymoc_hip.h -- C-ABI of libpymoc_hip.so, the MI355X (gfx950) engine behind the
 * PyMOC timestep() path.
 *
 * The reference (pymoc 0.0.1rc5) has no FFI of its own: its boundary is the Python
 * object API of four classes.  Every entry point below therefore names the Python
 * method (reference file:line, relative to the reference checkout) whose arithmetic
 * it replaces; the ctypes binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only.  Pointers inside the pm_* batch
 *     structs are DEVICE pointers obtained from pm_malloc(); everything else
 *     (the struct itself, host buffers of pm_memcpy_*) lives in host memory.
 *   - all floating point data is IEEE fp64; index/flag data is int32.
 *   - batches are "ensemble-major": a field of a batch of n independent members is
 *     one dense array [n][nlev], level fastest.
 *   - every function returns PM_OK (0) or an error code; pm_last_error() gives the
 *     text.  Kernel launches are asynchronous on the given stream (NULL = the
 *     library's default stream); pm_stream_sync / pm_memcpy_d2h are sync points.
 *   - no host pointer is retained after a call returns.
 */
#ifndef PYMOC_HIP_H
#define PYMOC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PM_OK 0
#define PM_EINVAL 1     /* bad argument (shape, NULL pointer, unsupported size)  */
#define PM_EHIP 2       /* a HIP runtime call failed                              */
#define PM_ENCCL 3      /* an RCCL call failed / librccl could not be loaded      */
#define PM_ENODEV 4     /* no HIP device visible                                  */

typedef void *pm_stream_t;
typedef void *pm_event_t;
typedef void *pm_comm_t;
typedef void *pm_graph_t;

/* ------------------------------------------------------------------ runtime */
const char *pm_version(void);
const char *pm_last_error(void);
int pm_device_count(int *count);
int pm_set_device(int device);
int pm_device_info(char *name, size_t name_len, int *compute_units,
                   size_t *hbm_bytes, int *clock_mhz);

int pm_malloc(void **dptr, size_t bytes);
int pm_free(void *dptr);
int pm_memset(void *dptr, int value, size_t bytes, pm_stream_t stream);
int pm_memcpy_h2d(void *dst, const void *src, size_t bytes, pm_stream_t stream);
int pm_memcpy_d2h(void *dst, const void *src, size_t bytes, pm_stream_t stream);
int pm_memcpy_d2d(void *dst, const void *src, size_t bytes, pm_stream_t stream);
/* Page-locked host memory and a device-to-host copy that does NOT synchronise: the copy is
 * ordered on `stream`, the caller reads `dst` after pm_stream_sync / pm_event_sync.  `dst` must
 * come from pm_host_alloc and stay alive until then (the one exception to "no host pointer is
 * retained": the caller owns the buffer and the sync point).  Used by the diagnostic time
 * series, which the reference fills every Diag_iters steps
 * (examples/run_JansenNadeau_2018.py:192-198, 218-226) and reads after the loop (:268-272).   */
int pm_host_alloc(void **hptr, size_t bytes);
int pm_host_free(void *hptr);
int pm_memcpy_d2h_async(void *dst_pinned, const void *src, size_t bytes, pm_stream_t stream);

/* Row gather on the device: for every item k < nitems (<= PM_PACK_MAX_ITEMS) and row r < nrows
 *   items[k].dst[r][0:nlev] = items[k].src[ sel ? sel[r] : r ][0:nlev]
 * (src rows `src_stride` doubles apart, dst rows dense), ONE launch.  `sel` is a device array
 * of int32 row numbers or NULL.  This is how a diagnostic sample -- the reference's
 * `AMOC_save[:, k] = AMOC.Psi`, ... of run_JansenNadeau_2018.py:219-225 -- is appended to the
 * device-resident time series (selected members only), and how the per-rank send buffer of the
 * diagnostic exchange is packed.                                                             */
#define PM_PACK_MAX_ITEMS 8
typedef struct pm_row_copy {
  const double *src;   /* [.][src_stride] */
  double *dst;         /* [nrows][nlev]   */
  int32_t nlev;
  int32_t src_stride;
} pm_row_copy;
int pm_rows_pack(const pm_row_copy *items, int32_t nitems, const int32_t *sel, int32_t nrows,
                 pm_stream_t stream);

int pm_stream_create(pm_stream_t *stream);
/* priority > 0: the device's highest stream priority (its workgroups are dispatched before those
   of normal streams when both have work pending), 0: as pm_stream_create */
int pm_stream_create_priority(pm_stream_t *stream, int priority);
int pm_stream_destroy(pm_stream_t stream);
int pm_stream_sync(pm_stream_t stream);
int pm_device_sync(void);

int pm_event_create(pm_event_t *event);
int pm_event_destroy(pm_event_t event);
int pm_event_record(pm_event_t event, pm_stream_t stream);
int pm_event_sync(pm_event_t event);
/* work submitted to `stream` after this call waits for `event` (hipStreamWaitEvent): lets two
 * independent launches -- Psi_SO.solve and Psi_Thermwind of one overturning update -- run side
 * by side on two streams and join before the columns step                                    */
int pm_stream_wait_event(pm_stream_t stream, pm_event_t event);
int pm_event_elapsed_ms(pm_event_t start, pm_event_t stop, float *ms);

/* hipGraph capture of a launch sequence issued on `stream` */
int pm_graph_begin_capture(pm_stream_t stream);
int pm_graph_end_capture(pm_stream_t stream, pm_graph_t *graph);
int pm_graph_launch(pm_graph_t graph, pm_stream_t stream);
int pm_graph_destroy(pm_graph_t graph);

/* ------------------------------------------------------------------ Column
 * Replaces pymoc.modules.Column time stepping:
 *   Column.convect       src/pymoc/modules/column.py:251-271
 *   Column.vertadvdiff   src/pymoc/modules/column.py:210-249
 *   Column.horadv        src/pymoc/modules/column.py:288-313
 *   Column.timestep      src/pymoc/modules/column.py:315-348  (order: convect,
 *                        vertadvdiff, horadv)
 * A batch is ncols independent columns on ONE shared vertical grid z[nz].
 */
#define PM_COL_DO_CONV 1   /* per-column flag: timestep(do_conv=True)             */
#define PM_COL_BZBOT 2     /* per-column flag: bzbot is not None (column.py:232)  */
#define PM_COL_STATIC_IN_RANGE 4 /* per-column HINT: z, kappa, Area, d(A kappa)/dz of every
                              coefficient set and bs / bbot / bzbot / N2min are finite and zero
                              or of magnitude in [2^-200, 2^200] (Area and the grid spacings not
                              zero).  The column kernels divide by static denominators with an
                              exact 4-instruction sequence that is IEEE-identical inside that
                              window; they test their operands and take IEEE division otherwise.
                              With the hint the one-step streaming kernel tests only what
                              changes from launch to launch (b, wA); without it, everything.   */
#define PM_COL_UNIFORM_AREA 8 /* per-column HINT: Area(z) is constant in z (every reference script);
                              the column kernels (G = 64) then read area[col][0] only.  Not
                              verified (that would be the read it saves): a wrong hint gives the
                              result for Area = area[col][0].                                   */

#define PM_OP_CONVECT 1      /* run convect() on columns flagged PM_COL_DO_CONV   */
#define PM_OP_VERTADVDIFF 2  /* run vertadvdiff(wA, dt, do_conv=flag)             */
#define PM_OP_HORADV 4       /* run horadv(vdx_in, b_in, dt)                      */
#define PM_OP_TIMESTEP 7     /* what Column.timestep does (horadv iff vdx given)  */
#define PM_OP_WEFF 8         /* modifier: the `wA` argument holds weff = wA - d(A kappa)/dz of
                                the coefficient set in use (pm_column_weff), which is all the step
                                needs of the two (column.py:241); d(A kappa)/dz is then not read.
                                wA is static between two overturning updates in every reference
                                driver, so weff is too.                                          */
#define PM_OP_WA_PSI 32      /* modifier for two-column ensembles (rows [0, ncols/2) basin, [ncols/2,
                                ncols) north): the `wA` argument holds the isopycnal overturning
                                Psi_iso [ncols][nz] in Sv and `b_in` (horadv's slot, no horadv with
                                this modifier) Psi_SO [ncols/2][nz] or NULL; the kernel forms the
                                drivers' forcing itself, wA_basin = (Psi_iso - Psi_SO) * 1e6,
                                wA_north = -Psi_iso * 1e6 (example_twocol_plusSO.py:105-106) --
                                what pm_thermwind_update's wA1 / wA2 outputs hold, without the
                                thermal wind having to wait for Psi_SO.  Launches of >= 3 steps. */
#define PM_OP_WA_TWOBASIN 64 /* modifier for the two-basin driver's three-column ensembles (rows [0, n)
                                Atlantic, [n, 2n) north, [2n, 3n) Pacific, n = ncols / 3): `wA` holds the
                                AMOC's isopycnal overturnings [2n][nz] (rows [0, n) on the Atlantic
                                column, [n, 2n) on the northern one), `vdx_in` (horadv's slot: no horadv
                                with this modifier) the zonal overturning's [2n][nz] (Atlantic, Pacific)
                                and `b_in` the two sectors' Psi_SO [2n][nz] (Atlantic, Pacific), all
                                in Sv; the kernel forms the driver's forcing itself,
                                  wA_Atl = (iso_A + zon_A - SO_A) * 1e6,  wA_north = -iso_N * 1e6,
                                  wA_Pac = (-zon_P - SO_P) * 1e6   (twobasin_NadeauJansen.py:103-105)
                                -- pm_twobasin_forcing's operations, without that launch.  Each of
                                the three arrays is read in its 2n rows only (a Pacific column takes
                                nothing from `wA`).  Launches of >= 3 steps.                       */
#define PM_OP_CONTRACTED 16  /* modifier, OPT-IN tolerance mode: launches of >= 3 plain timesteps
                                (one wave per column, nz <= 256) use the contracted update
                                b_i += cu_i (b_{i+1}-b_i) + cl_i (b_i-b_{i-1}) with per-launch
                                coefficients instead of the reference's operation order (3
                                instead of 21 instructions per level).  Agrees with the reference
                                to rounding (<= 1e-12 relative over BASELINE's runs), not bit for
                                bit; without the flag every result is bit-identical to NumPy.    */

#define PM_COLS_ALL_UNIFORM_AREA 1 /* pm_columns.reserved, batch-wide HINT: EVERY column carries
                              PM_COL_UNIFORM_AREA.  With it, PM_OP_WEFF and kappa_base /
                              kappa_profile a one-step launch on a large batch keeps only b and
                              weff of a column in flight (24 nz B per column-step)               */

#define PM_COLS_DIV3_PROVEN 2 /* pm_columns.reserved, batch-wide HINT (with PM_COLS_ALL_UNIFORM_AREA): the
                              caller has established with pm_div3_proven() that EVERY static
                              denominator of the batch's column step -- the grid spacings z[i+1] -
                              z[i], the centred spacings 0.5 ((z[i+1] - z[i]) + (z[i] - z[i-1])) and
                              every column's Area -- admits the 3-instruction exact quotient
                              (below).  Fused launches then divide in 3 instead of 4 instructions;
                              results are bit-identical (the quotient is the IEEE one).           */

#define PM_COLS_DIV2_GRID 4 /* pm_columns.reserved, batch-wide HINT, honoured only together with
                              PM_COLS_DIV3_PROVEN (ignored otherwise): pm_div2_proven() and
                              pm_recip2_check() hold for every grid spacing and centred spacing of
                              the batch, so the fused launch divides by them with the 2-instruction
                              exact quotient (below).  Bit-identical results.                     */
#define PM_COL_DIV2_AREA 16 /* per-column HINT (pm_columns.flags), honoured only together with
                              PM_COLS_DIV3_PROVEN and PM_COLS_DIV2_GRID: pm_div2_proven() and
                              pm_recip2_check() hold for this column's Area, so all three of its
                              quotients take the 2-instruction form.  A column without it keeps
                              the 3-instruction quotient for the division by Area.                */

typedef struct pm_columns {
  int32_t ncols;         /* independent columns in the batch                      */
  int32_t nz;            /* levels per column (2 <= nz <= 1024)                   */
  int32_t nsel;          /* coefficient sets per column (1, or 2 for JN2018)      */
  int32_t reserved;      /* batch-wide hint bits (PM_COLS_*), else 0              */
  const double *z;       /* [nz]              shared grid, ascending              */
  double *b;             /* [ncols][nz]       buoyancy, updated in place          */
  const double *kappa;   /* [nsel][ncols][nz] kappa(z)                            */
  const double *area;    /* [ncols][nz]       Area(z)                             */
  const double *dAkappa; /* [nsel][ncols][nz] np.gradient(Area*kappa, z)          */
  const double *bs;      /* [ncols] surface buoyancy                              */
  const double *bbot;    /* [ncols] bottom buoyancy (used unless PM_COL_BZBOT)    */
  const double *bzbot;   /* [ncols] bottom stratification (may be NULL)           */
  const double *N2min;   /* [ncols] convective-adjustment stratification          */
  const int32_t *flags;  /* [ncols] PM_COL_* bits                                 */
  const int32_t *ksel;   /* [ncols] coefficient set in use (NULL -> set 0)        */
  int32_t *nonfinite;    /* [ncols] out: 1 if b holds a non-finite value at the
                            end of the call (NULL -> not reported)                */
  const double *kappa_base;    /* [ncols] or NULL */
  const double *kappa_profile; /* [nz] or NULL.  Both given (nsel = 1): a HINT that
                            kappa[col][i] == kappa_base[col] + kappa_profile[i] BIT FOR BIT (one
                            fp64 addition) -- a parameter sweep over a background diffusivity, the
                            kappa sweep of BASELINE's ensembles.  Launches that stream the
                            coefficient arrays (one or two steps per launch on a large batch) then
                            FORM kappa instead of reading it: with PM_OP_WEFF 24 nz B per
                            column-step (b and weff in, b out: SURVEY 8d's algorithmic bytes) instead
                            of 32 nz.  The caller vouches for the identity (the Python ColumnBatch
                            verifies it on the host arrays); other launches read kappa as ever.  */
} pm_columns;

/* nsteps repetitions of the selected ops with wA (and vdx_in/b_in) held fixed, the
 * whole loop fused in one launch with b resident in registers.
 *   wA      [ncols][nz]  m^3/s
 *   vdx_in  [ncols][nz]  or NULL; b_in [ncols][nz] required when vdx_in given
 *   lanes_per_col  16, 32 or 64 lanes cooperate on one column; 0 = choose        */
int pm_column_steps(const pm_columns *cols, const double *wA, const double *vdx_in,
                    const double *b_in, double dt, int32_t nsteps, int32_t ops,
                    int32_t lanes_per_col, pm_stream_t stream);

/* Backward-Euler column steps: an EXTENSION with no reference counterpart (the reference's
 * vertadvdiff, column.py:210-249, is forward Euler and unstable above kappa dt / dz^2 = 1/2), so a
 * TOLERANCE path: bit-identical to nothing but itself (nsteps = k in one launch equals k launches of
 * one step, bit for bit).  With the reference's discretisation -- dz = z[1:] - z[:-1],
 * dzc_i = 0.5 (dz[i] + dz[i-1]), w_i = weff_i / Area_i (weff = wA - d(A kappa)/dz, the upwind test
 * `w_i < 0` the reference's own) --
 *   cl_i = (w_i < 0 ? 0 : w_i / dz[i-1]) + kappa_i / (dzc_i dz[i-1])
 *   cu_i = (w_i < 0 ? -w_i / dz[i] : 0)  + kappa_i / (dzc_i dz[i])
 * one step is: convect() (PM_OP_CONVECT, columns flagged PM_COL_DO_CONV: the explicit kernel's device
 * function, same bits); b[nz-1] = bs unless the column is flagged PM_COL_DO_CONV; b[0] = bbot; solve
 *   (1 + dt (cl_i + cu_i)) x_i - dt cl_i x_{i-1} - dt cu_i x_{i+1} = b_i,   i = 1 .. nz-2
 * (one strictly diagonally dominant tridiagonal system per column, no pivoting; under PM_COL_BZBOT
 * x_0 = x_1 - bzbot dz[0] is folded into row 1 and b[0] = x_1 - bzbot dz[0] afterwards); store x.
 * The matrix is factored once per launch.  Reads pm_columns as pm_column_steps does (ksel / nsel,
 * per-column flags, nonfinite); the exact-division hints are ignored.  wA [ncols][nz] may be NULL
 * (= 0).  ops: PM_OP_CONVECT | PM_OP_VERTADVDIFF, optionally PM_OP_WEFF; PM_OP_HORADV,
 * PM_OP_CONTRACTED, PM_OP_WA_PSI, PM_OP_WA_TWOBASIN, nsteps < 0 and a dt that is not finite and
 * positive are PM_EINVAL; nsteps == 0 launches nothing.                                          */
int pm_column_steps_implicit(const pm_columns *cols, const double *wA, double dt, int32_t nsteps,
                             int32_t ops, pm_stream_t stream);

/* pm_column_steps_implicit for the two-basin driver's three-column ensembles (rows [0, n) Atlantic,
 * [n, 2n) north, [2n, 3n) Pacific, n = ncols / 3), the forcing formed by the kernel itself as it
 * builds the matrix, from the AMOC's isopycnal overturnings `iso` [2n][nz] (Atlantic, north), the
 * zonal overturning's `zon` [2n][nz] (Atlantic, Pacific) and the two sectors' Psi_SO `so` [2n][nz]
 * (Atlantic, Pacific), all in Sv:
 *   wA_Atl = (iso_A + zon_A - SO_A) * 1e6,  wA_north = -iso_N * 1e6,  wA_Pac = (-zon_P - SO_P) * 1e6
 * (twobasin_NadeauJansen.py:103-105) -- pm_twobasin_forcing's operations in its order.  Like its
 * sibling an extension and a TOLERANCE path against the reference; against the sibling it is
 * bit-identical: the result equals pm_twobasin_forcing into an array followed by
 * pm_column_steps_implicit on that array, for every nsteps >= 1.  Each array is read in its 2n rows
 * only (a Pacific column takes nothing from `iso`).  ops: PM_OP_CONVECT | PM_OP_VERTADVDIFF
 * (PM_OP_WA_TWOBASIN is implied and may be given).  PM_EINVAL: ncols not a multiple of 3, one of the
 * three arrays NULL on a non-empty batch, PM_OP_WEFF, PM_OP_HORADV, PM_OP_CONTRACTED, PM_OP_WA_PSI
 * or unknown op bits, nsteps < 0, a dt that is not finite and positive, nz outside [2, 1024].  An
 * empty batch and nsteps == 0 launch nothing.                                                     */
int pm_column_steps_implicit_twobasin(const pm_columns *cols, const double *iso, const double *zon,
                                      const double *so, double dt, int32_t nsteps, int32_t ops,
                                      pm_stream_t stream);

/* weff[ncols][nz] = wA - d(A kappa)/dz of each column's coefficient set in use (column.py:241),
 * for pm_column_steps(..., ops | PM_OP_WEFF).                                                 */
int pm_column_weff(const pm_columns *cols, const double *wA, double *weff, pm_stream_t stream);

/* The work decomposition pm_column_steps would use for a batch of this shape: lanes
 * cooperating on one column (`lanes_per_col` = 0 lets the library choose) and levels held
 * per lane; reporting only (bench.py names the kernel instantiation with it).            */
int pm_column_kernel_shape(int32_t ncols, int32_t nz, int32_t lanes_per_col,
                           int32_t *lanes, int32_t *levels_per_lane);
/* Name of the kernel instantiation pm_column_steps launches for these arguments (reporting
 * only), spelled as profilers report it with every template argument:
 * "k_column_steps<G,P,FAST,PLAIN,UA>", or for 1-2 steps on a large ensemble
 * "k_column_stream<P,D,AFF,LEAN,VEC,D3,CPWU,WEFFT,UABT>"; "" when the call launches nothing.
 * The same checks as pm_column_steps (b_in aside); no pointer is dereferenced, but the batch's
 * hint bits, kappa_base / kappa_profile and the alignment of b and wA steer the choice.      */
int pm_column_kernel_name(const pm_columns *cols, const double *wA, const double *vdx_in,
                          int32_t nsteps, int32_t ops, int32_t lanes_per_col, char *name,
                          size_t name_len);
/* *twin = 1 when pm_column_steps with these arguments runs k_column_steps_cls, the twin of the
 * one-wave-per-column uniform-Area rows (G = 64, at most 2 levels per lane, plain timesteps) that
 * launches of at least 64 steps take; 0 otherwise, and when the call launches nothing.
 * pm_column_kernel_name reports the row's name either way.  The same checks, reporting only.  */
int pm_column_kernel_twin(const pm_columns *cols, const double *wA, const double *vdx_in,
                          int32_t nsteps, int32_t ops, int32_t lanes_per_col, int32_t *twin);

/* ------------------------------------------------------------------ Psi_Thermwind
 * Replaces pymoc.modules.Psi_Thermwind for n independent members on one grid z[nz]:
 *   Psi_Thermwind.solve  src/pymoc/modules/psi_thermwind.py:125-135  (PM_TW_SOLVE)
 *   Psi_Thermwind.Psib   src/pymoc/modules/psi_thermwind.py:137-185  (PM_TW_PSIB)
 *   Psi_Thermwind.Psibz  src/pymoc/modules/psi_thermwind.py:187-208  (PM_TW_PSIBZ,
 *                        needs PM_TW_PSIB in the same call)
 * and, optionally, the drivers' coupling to the columns (examples/example_twocol.py
 * :87-88, example_twocol_plusSO.py:105-106): wA1 = (psibz1 - Psi_SO)*1e6 (Psi_SO NULL
 * -> psibz1*1e6), wA2 = -psibz2*1e6.  Without PM_TW_SOLVE, Psi is an input.          */
#define PM_TW_SOLVE 1
#define PM_TW_PSIB 2
#define PM_TW_PSIBZ 4
#define PM_TW_WA_PSI 8 /* with PM_TW_SOLVE: wA1 = Psi*1e6 (example_timestepping.py:75) */

typedef struct pm_thermwind {
  int32_t n;            /* members                                               */
  int32_t nz;           /* levels (2 <= nz <= 1024)                              */
  int32_t nb;           /* isopycnal classes of Psib (reference default 500)     */
  int32_t reserved;
  const double *z;      /* [nz]    shared grid                                   */
  const double *b1;     /* [n][nz] buoyancy of the basin column                  */
  const double *b2;     /* [n][nz] buoyancy of the northern column               */
  const double *f;      /* [n]     Coriolis parameter                            */
  double *Psi;          /* [n][nz] overturning, Sv (out with PM_TW_SOLVE, else in)*/
  double *bgrid;        /* [n][nb] out, may be NULL                              */
  double *psib;         /* [n][nb] out, may be NULL.  With bgrid AND psib NULL and PM_TW_PSIBZ
                           a member whose upstream cells lie in chain order sums only the
                           classes Psibz's interpolations read (70-135 of 500 on BASELINE's
                           ensembles): psibz1 / psibz2 / wA1 / wA2 are the same bits either way */
  double *psibz1;       /* [n][nz] out, may be NULL                              */
  double *psibz2;       /* [n][nz] out, may be NULL                              */
  const double *Psi_SO; /* [n][nz] in, may be NULL                               */
  double *wA1;          /* [n][nz] out, may be NULL                              */
  double *wA2;          /* [n][nz] out, may be NULL                              */
  const double *b1_mid; /* [n][nz] b1 at the midpoints z[k] + (z[k+1]-z[k])/2 of the     */
  const double *b2_mid; /*         intervals, for CALLABLE profiles (solve_bvp evaluates */
                        /*         them there); NULL = linear between the levels        */
  double *dPsi;         /* [n][nz] out with PM_TW_SOLVE, may be NULL: d(Psi 1e6)/dz at the  */
                        /*         levels (the second component of solve_bvp's solution)    */
} pm_thermwind;

int pm_thermwind_update(const pm_thermwind *tw, int32_t ops, pm_stream_t stream);

/* solve_bvp's rms residual of every interval of ONE member's mesh x[m] (scipy 1.15.3
 * _bvp.py:estimate_rms_residuals: 5-point Lobatto rule on the C1 cubic spline of (y, f)) for the
 * thermal-wind problem y0' = y1, y1' = g(x): y0[m] = Psi (in Sv, as stored) and y1[m] = dPsi from
 * pm_thermwind_update on the mesh, g[m] = (b2 - b1)/f at the nodes, g_lob[2][m-1] at the two
 * inner Lobatto points x_mid +- h sqrt(3/7)/2 of every interval (CALLABLE profiles: sampled by
 * the host, which owns solve_bvp's mesh loop: pymoc_amd/modules/psi_thermwind.py).  rms[m-1].  */
int pm_thermwind_residuals(int32_t m, const double *x, const double *y0, const double *y1,
                           const double *g, const double *g_lob, double *rms,
                           pm_stream_t stream);

/* ------------------------------------------------------------------ Psi_SO
 * Replaces pymoc.modules.Psi_SO for n independent members on shared grids z[nz], y[ny]:
 *   Psi_SO.ys          src/pymoc/modules/psi_SO.py:106-140
 *   Psi_SO.calc_Ekman  src/pymoc/modules/psi_SO.py:218-243   (PM_SO_OP_EKMAN)
 *   Psi_SO.calc_GM     src/pymoc/modules/psi_SO.py:277-331   (PM_SO_OP_GM; without
 *                      PM_SO_OP_EKMAN it reads Psi_Ek as the caller's self.Psi_Ek)
 *   Psi_SO.solve       src/pymoc/modules/psi_SO.py:333-354   (PM_SO_OP_SOLVE)
 * Scalar options of the constructor are shared by the batch; KGM and tau vary per member. */
#define PM_SO_HAS_C 1          /* c is not None: F2010 boundary-value smoother       */
#define PM_SO_BVP_WITH_EK 2
#define PM_SO_HAS_HSILL 4
#define PM_SO_HAS_HEK 8
#define PM_SO_HAS_HTAPERTOP 16
#define PM_SO_HAS_HTAPERBOT 32
#define PM_SO_TAU_ARRAY 64     /* tau is [n][ny] on y instead of one scalar per member */
#define PM_SO_NO_FIXUP 128     /* do not issue the follow-up launch of the adaptive GM mesh: members
                                  whose mesh outgrew the register solver stay flagged in `status`
                                  (bit 3) with the 256-node solution                            */

#define PM_SO_OP_EKMAN 1
#define PM_SO_OP_GM 2
#define PM_SO_OP_SOLVE 3

typedef struct pm_psi_so {
  int32_t n, nz, ny, flags;
  int32_t bvp_refine;   /* GM BVP mesh: 0 / -1 = follow scipy solve_bvp's own adaptive mesh
                           (1e-14 from the reference); R > 0 = fixed R-fold refinement
                           of the column grid (2-3x faster, ~1e-6 from the reference)   */
  int32_t reserved;
  const double *z;      /* [nz] */
  const double *y;      /* [ny] */
  const double *b;      /* [n][nz] basin buoyancy at the northern end of the channel */
  const double *bs;     /* [n][ny] surface buoyancy                                  */
  const double *tau;    /* [n] or, with PM_SO_TAU_ARRAY, [n][ny]                     */
  const double *KGM;    /* [n] */
  double f, rho, L, smax, c, Hsill, HEk, Htapertop, Htaperbot;
  double *Psi;          /* [n][nz] out, Sv                                           */
  double *Psi_Ek;       /* [n][nz] out, Sv (in when PM_SO_OP_GM alone)               */
  double *Psi_GM;       /* [n][nz] out, Sv                                           */
  double *Ek_raw;       /* [n][nz] out, m^3/s: calc_Ekman() return value (may be NULL)*/
  double *GM_raw;       /* [n][nz] out, m^3/s: calc_GM() return value (may be NULL)  */
  double *ys;           /* [n][nz] out: outcrop latitude of b[i] (may be NULL)        */
  int32_t *status;      /* [n] out: bit0 bs not monotone north of its minimum (several
                           roots: ys then follows brentq's own iteration, like the
                           reference), bit1 non-finite Psi, bit2 NaN in bs, bit3 the adaptive GM
                           mesh would exceed solve_bvp's own max_nodes = 1000 (it stops
                           there too; the solution of the last mesh is returned).  For
                           nz <= 128 the first launch follows meshes up to 256 nodes and
                           a follow-up launch redoes the members it flagged, which needs
                           `status` (without it bit 3 semantics cannot be repaired and
                           the 256-node solution stands) (may be NULL)                   */
  const double *ys_in;      /* [n][nz] optional: outcrop latitudes computed by the caller   */
  const double *tau_ave_in; /* [n][nz] optional: wind stress averaged from ys to y[-1].
                               For CALLABLE bs / tau, which only the host can evaluate: the
                               drop-in class root-finds and averages exactly like the
                               reference (psi_SO.py:106-140, :238-240) and hands the results
                               in; both NULL = computed on the device from bs[n][ny], tau  */
} pm_psi_so;

int pm_psi_so_update(const pm_psi_so *so, int32_t ops, pm_stream_t stream);

/* ------------------------------------------------------------------ SO_ML
 * Replaces pymoc.modules.SO_ML.timestep / advdiff (src/pymoc/modules/SO_ML.py:198-303,
 * with set_boundary_conditions :77-98, calc_advective_tendency :100-134 and the
 * Crank-Nicolson calc_implicit_diffusion :136-196 as a Thomas sweep) for n members on a
 * shared uniform grid y[ny]; the basin profiles live on z with nz levels.               */
typedef struct pm_so_ml {
  int32_t n, nz, ny, reserved;
  const double *y;         /* [ny] uniform meridional grid                            */
  double *bs;              /* [n][ny] mixed-layer buoyancy, updated in place           */
  double *Psi_s;           /* [n][ny] out: overturning at the surface, Sv (may be NULL) */
  const double *b_basin;   /* [n][nz] buoyancy of the adjoining basin                  */
  const double *Psi_b;     /* [n][nz] SO overturning on the basin's levels, Sv         */
  const double *surflux;   /* [n][ny] */
  const double *rest_mask; /* [n][ny] */
  const double *b_rest;    /* [n][ny] */
  double Ks, h, L, v_pist;
  int32_t *status;         /* [n] out: 1 where the reference raises IndexError (Psi_b all
                              zero / no upwelling level; state left untouched), 2 non-finite
                              result, 16 (pm_jn2018_steps only) a wrong
                              PM_JN_UNIFORM_AREA hint, 32 (pm_jn2018_steps' uniform-Area
                              kernel only) an operand of the column steps -- state, forcing,
                              coefficients, grid, dt -- outside the window [2^-200, 2^200] in
                              which the kernel's 4-instruction division is IEEE-identical: the
                              member's steps from there on were taken by the call's follow-up
                              launch with true divisions (the reference's arithmetic for any
                              operand, like pm_column_steps' own fallback); informational.
                              Bits 8.. are scratch of that hand-over and are cleared by it
                              (may be NULL: pm_jn2018_steps then uses its general kernel)   */
} pm_so_ml;

int pm_so_ml_step(const pm_so_ml *ml, double dt, pm_stream_t stream);

/* Per-step bottom boundary condition and bottom-boundary-layer diffusivity selection of the
 * Jansen & Nadeau driver, examples/run_JansenNadeau_2018.py:233-254.  Columns are stored
 * basin rows [0, n) then north rows [n, 2n); coefficient set 0 = kappa, 1 = kappaeff.    */
typedef struct pm_jn2018_bc {
  int32_t n, nz, ny, reserved;
  const double *Psi_SO;    /* [n][nz] PsiSO.Psi                                        */
  const double *Psi_res_b; /* [n][nz] AMOC.Psibz()[0]                                  */
  const double *Psi_res_n; /* [n][nz] AMOC.Psibz()[1]                                  */
  const double *b_basin;   /* [n][nz] */
  const double *b_north;   /* [n][nz] */
  const double *bs_SO;     /* [n][ny] channel.bs                                       */
  double *bbot;            /* [2n] in/out: Column.bbot of basin / north columns        */
  int32_t *ksel;           /* [2n] in/out: coefficient set of basin / north columns    */
} pm_jn2018_bc;

int pm_jn2018_bc_switch(const pm_jn2018_bc *bc, pm_stream_t stream);

/* Fused Jansen & Nadeau time loop (examples/run_JansenNadeau_2018.py:228-261): nsteps x
 * [bottom-BC switch -> basin.timestep(do_conv) -> north.timestep(do_conv) ->
 * channel.timestep] per member in ONE launch, with wA / Psi_SO / Psibz held fixed (they only
 * change at MOC updates, :204-217).  Bit-identical to issuing pm_jn2018_bc_switch +
 * pm_column_steps + pm_so_ml_step per step.  `cols` holds 2n columns (basin rows [0,n),
 * north rows [n,2n), nsel = 2, bbot / ksel updated in place); `ml.b_basin` / `ml.Psi_b` are
 * ignored (the basin column and Psi_SO are used).  nz <= 256.                          */
#define PM_JN_UNIFORM_AREA 1 /* hint: Area(z) of every column is constant in z (true for every
                                reference script); a kernel variant then keeps it in scalar
                                registers.  A wrong hint is detected: the launch fails the
                                members' status with bit 4 (16) and leaves them untouched.  */
#define PM_JN_CONTRACTED 2   /* OPT-IN tolerance mode of the uniform-Area kernel: the two columns
                                step in the contracted form of PM_OP_CONTRACTED (agreement with
                                the reference to rounding, not bit for bit; the mixed layer and
                                the bottom-BC switch keep the reference's operation order)     */
#define PM_JN_SHARED_COEF 4  /* hint of the uniform-Area kernel: the kappa / dAkappa / Area rows of
                                every basin column equal basin column 0's and those of every
                                northern column equal northern column 0's (a parameter sweep
                                over forcing and boundary values, as run_JansenNadeau_2018.py's
                                parameters are: one kappa(z) for all members).  The kernel then
                                reads only rows 0 and n -- they stay in L2 -- instead of six rows
                                per member from HBM.  The CALLER vouches for it (verifying it on
                                the device would read the rows it is meant to save); the Python
                                driver compares the host arrays.                                */
#define PM_JN_SPLIT_LANES 8  /* OPT-IN lane layout of the uniform-Area kernel (round 5): the two
                                columns of a member step together, basin on lanes 0..31 and
                                north on lanes 32..63 with ceil(nz/32) levels per lane, instead
                                of one after the other on 64 lanes each.  Same arithmetic per
                                level, bit-identical results; 65 <= nz <= 128 or 193 <= nz <= 224,
                                other shapes ignore the hint.                                  */
#define PM_JN_DIV3_PROVEN 16 /* hint of the uniform-Area kernel: pm_div3_proven and pm_recip_check hold
                              for every static denominator of the fused loop -- the grid spacings and
                              centred spacings of z, both columns' Area of every member, and the
                              mixed layer's h, L and y[1] - y[0]: its quotients then take 3 instead
                              of 4 instructions (bit-identical)                                    */
typedef struct pm_jn2018 {
  int32_t n, hints, reserved1, reserved2;
  pm_columns cols;
  const double *wA;        /* [2n][nz] */
  const double *Psi_SO;    /* [n][nz]  */
  const double *Psi_res_b; /* [n][nz]  */
  const double *Psi_res_n; /* [n][nz]  */
  pm_so_ml ml;
} pm_jn2018;

int pm_jn2018_steps(const pm_jn2018 *jn, double dt, int32_t nsteps, pm_stream_t stream);

/* The same fused loop (examples/run_JansenNadeau_2018.py:229-261) with both columns advanced by
 * backward Euler: an EXTENSION, no reference counterpart (the script's columns are forward Euler,
 * which at its own nz = 200 cannot take its dt = 30 d).  Exactly nsteps x
 *   [pm_jn2018_bc_switch;
 *    pm_column_steps_implicit(cols, wA, dt, 1, PM_OP_CONVECT | PM_OP_VERTADVDIFF) on the 2n columns;
 *    pm_so_ml_step with b_basin = the basin rows, Psi_b = Psi_SO]
 * per member in ONE launch, wA / Psi_SO / Psi_res_b / Psi_res_n held fixed, and bit-identical to
 * that launch sequence: b, ml.bs, ml.Psi_s, bbot, ksel, cols.nonfinite (each column's own flag)
 * and ml.status (the last step's: 1 where the mixed layer did not step, else 2 where ml.bs is not
 * finite).  A column's matrix is factored at launch and again only in a step whose BC switch
 * changes its coefficient set.  2 <= nz <= 256, any ny pm_so_ml_step takes within the CU's LDS,
 * Area per level.  PM_JN_CONTRACTED, PM_JN_SPLIT_LANES, nsteps < 0 and a dt that is not finite and
 * positive are PM_EINVAL; the other hints are ignored; n == 0 or nsteps == 0 launches nothing.  */
int pm_jn2018_steps_implicit(const pm_jn2018 *jn, double dt, int32_t nsteps, pm_stream_t stream);

/* ------------------------------------------------------------------ whole coupled runs
 * The reference's coupled drivers are loops "every MOC_up_iters steps refresh the overturning
 * diagnostics, then step" (examples/example_twocol.py:85-96, run_JansenNadeau_2018.py:201-261).
 * pm_twocol_run / pm_jn2018_run carry every member through MANY such intervals in ONE launch:
 * a wavefront owns a member and runs the diagnostic phase and the stepping phase of each
 * interval back to back (members never interact, so no launch boundary is needed between
 * them).  The phases are the device functions of pm_psi_so_update, pm_thermwind_update and
 * pm_jn2018_steps / pm_column_steps, so the result is bit-identical to issuing those calls in
 * the drivers' order.  Schedule of one launch:
 *     n_first steps;  then n_updates x [refresh the diagnostics; steps], where the last block
 *     steps n_last (possibly 0) and the others m_steps.
 * A driver ends a launch where it wants to look at the state (diagnostic output, RCCL gather). */
typedef struct pm_run_schedule {
  int32_t n_first, n_updates, m_steps, n_last;
} pm_run_schedule;

/* example_twocol.py:85-96: per member a basin column (row m of `cols`) and a northern column
 * (row n + m), Psi_Thermwind solve / Psib / Psibz between them (`tw`: b1 = cols.b, b2 = cols.b +
 * n nz; wA1 = wA, wA2 = wA + n nz; psibz1 / psibz2 / Psi are outputs; Psi_SO NULL), forcing
 * wA[2n][nz] (in for the n_first steps, rewritten by every refresh).  Requires: Area constant in
 * z, no bzbot, nz <= 256 with (7 nz' + 16 max(...)) doubles of LDS <= 160 KB (checked).
 * status[n] (must be zeroed by the caller; bits are OR-ed in): 2 non-finite state, 16 columns this
 * kernel cannot step (left untouched), 32 some interval stepped with IEEE divisions because an
 * operand was outside the exact-division window (same guard as pm_column_steps).            */
typedef struct pm_twocol_loop {
  pm_columns cols;
  pm_thermwind tw;
  const double *wA;
  double dt;
  pm_run_schedule sched;
  int32_t *status;
} pm_twocol_loop;
int pm_twocol_run(const pm_twocol_loop *run, pm_stream_t stream);

/* run_JansenNadeau_2018.py:201-261: per interval PsiSO.solve (`so`: b = the basin rows of jn.cols,
 * bs = jn.ml.bs, Psi = jn.Psi_SO), AMOC.solve / Psibz (`tw`: b1 / b2 = the basin / northern rows,
 * Psi_SO = jn.Psi_SO, wA1 / wA2 = jn.wA rows, psibz1 / psibz2 = jn.Psi_res_b / Psi_res_n), then the
 * fused step loop of pm_jn2018_steps.  `jn` as for pm_jn2018_steps with PM_JN_UNIFORM_AREA
 * (ny <= 64, 4 <= nz <= 256); `so` without the boundary-value smoother (c = None).
 * jn.ml.status as for pm_jn2018_steps, but OR-ed over the intervals (zero it first).        */
typedef struct pm_jn2018_loop {
  pm_jn2018 jn;
  pm_thermwind tw;
  pm_psi_so so;
  double dt;
  pm_run_schedule sched;
} pm_jn2018_loop;
int pm_jn2018_run(const pm_jn2018_loop *run, pm_stream_t stream);

/* One MOC update of the Jansen & Nadeau driver (run_JansenNadeau_2018.py:206-217) in ONE launch:
 * pm_psi_so_update(so, PM_SO_OP_SOLVE) followed by pm_thermwind_update(tw, tw_ops) for the same
 * members (same device functions, bit-identical results; `tw` may read so->Psi as its Psi_SO).
 * `so` without the boundary-value smoother (c = None), so->n == tw->n, so->nz == tw->nz <= 256.
 * Other shapes: PM_EINVAL -- issue the two calls.                                              */
int pm_so_tw_update(const pm_psi_so *so, const pm_thermwind *tw, int32_t tw_ops,
                    pm_stream_t stream);

/* LDS bytes per block (16 members) the phases of a run kernel need for this shape: kind 0 =
 * pm_twocol_run, 1 = pm_jn2018_run (ny: points of the mixed layer).  A launch is refused
 * (PM_EINVAL) above 160 KB; a driver asks first and keeps its launch sequence otherwise.
 * 0 = shape not supported at all.                                                           */
int pm_run_lds_bytes(int32_t kind, int32_t nz, int32_t nb, int32_t ny, size_t *bytes);

/* Column forcing of the two-column drivers as an array (what PM_OP_WA_PSI forms inside the
 * column kernel; for launches of fewer than 3 steps): wA[0:n] = (Psi_iso[0:n] - Psi_SO) * 1e6
 * (Psi_SO may be NULL), wA[n:2n] = -Psi_iso[n:2n] * 1e6; Psi_iso, wA [2n][nz], Psi_SO [n][nz]. */
int pm_twocol_forcing(int32_t n, int32_t nz, const double *Psi_iso, const double *Psi_SO,
                      double *wA, pm_stream_t stream);

/* Column forcing of the two-basin driver, examples/twobasin_NadeauJansen.py:103-105:
 *   wA_Atl = (Psi_iso_Atl + Psi_zonal_Atl - SO_Atl.Psi)*1e6
 *   wAN    = -Psi_iso_N*1e6
 *   wA_Pac = (-Psi_zonal_Pac - SO_Pac.Psi)*1e6          all arrays [n][nz]            */
int pm_twobasin_forcing(int32_t n, int32_t nz, const double *Psi_iso_Atl,
                        const double *Psi_zonal_Atl, const double *SO_Atl,
                        const double *Psi_iso_N, const double *Psi_zonal_Pac,
                        const double *SO_Pac, double *wA_Atl, double *wAN, double *wA_Pac,
                        pm_stream_t stream);

/* ---------------------------------------------------- equilibrium column
 * Column.solve_equi (src/pymoc/modules/column.py:187-208 with ode :161-164 and bc :124-159):
 * the steady advective-diffusive profile, which the reference obtains from
 * scipy.integrate.solve_bvp.  pm_column_equi_pass is ONE mesh pass of that solver for n
 * members, each on its own mesh: the exact solution of the 4th-order collocation system
 * (the ODE is linear), the rms residual estimate of every interval and the number of nodes
 * solve_bvp would insert.  The caller refines the flagged meshes and calls again until nadd
 * is 0 (pymoc_amd/equilibrium.py does, following solve_bvp's loop).
 * Point sets of a mesh x[m]: 0 = the m nodes; 1 = the m-1 interval middles x[i] + h/2;
 * 2 / 3 = the Lobatto points middle +- (h/2) sqrt(3/7).                                  */
typedef struct pm_column_equi {
  int32_t n, nz, mmax, reserved;
  const int32_t *m;       /* [n] mesh nodes of each member, 2 <= m <= mmax <= 1024        */
  const int32_t *active;  /* [n] 0 = skip this member (may be NULL: all active)           */
  const double *x;        /* [n][mmax] ascending mesh, contains every level of z          */
  const double *Ak;       /* [4][n][mmax] Column.Akappa at the four point sets            */
  const double *dAk;      /* [4][n][mmax] Column.dAkappa_dz at the four point sets        */
  const double *wA;       /* [4][n][mmax] wA at the four point sets, or NULL to use wA_z  */
  const double *wA_z;     /* [n][nz] wA on the column grid (np.interp'ed on the device)   */
  const double *z;        /* [nz] column grid (needed with wA_z)                          */
  const double *bs;       /* [n] */
  const double *bbot;     /* [n] */
  const double *bzbot;    /* [n] or NULL */
  const int32_t *flags;   /* [n] PM_COL_BZBOT: b'(-H) = bzbot replaces b(-H) = bbot (or NULL) */
  const int32_t *zidx;    /* [n][nz] position of column level k in the member's mesh      */
  double tol;             /* solve_bvp's tol (the reference uses the default 1e-3)        */
  double *y;              /* [n][2][mmax] out: b and db/dz on the mesh (may be NULL)      */
  double *rms;            /* [n][mmax] out: rms residual of every interval (may be NULL)  */
  int32_t *nadd;          /* [n] out: nodes solve_bvp would insert; 0 = converged (or NULL) */
  double *b;              /* [n][nz] out: Column.b on the column grid (may be NULL)       */
  double *bz;             /* [n][nz] out: Column.bz (may be NULL)                         */
} pm_column_equi;

int pm_column_equi_pass(const pm_column_equi *eq, pm_stream_t stream);

/* Equi_Column.solve (src/pymoc/modules/equi_column.py:408-435; ode :349-406, bc :286-347,
 * alpha :231-249, bz :251-284, non-dimensional profiles :116-185): the equilibrium overturning
 * of a basin as a 4th-order boundary-value problem on z* in [-1, 0], with the cell depth H
 * either given or an unknown parameter, which the reference solves with
 * scipy.integrate.solve_bvp.  pm_equi_column_newton is ONE mesh iteration of solve_bvp for n
 * members (each on its own mesh): solve_newton (forward-difference Jacobians, damped Newton,
 * <= 8 iterations / 4 Jacobians), the rms residual estimate of every interval, the number of
 * nodes solve_bvp would insert, and the largest boundary residual.  The caller owns
 * solve_bvp's outer loop (pymoc_amd/equi_column.py): insert nodes, transfer the solution to
 * the new mesh with the C1 cubic spline of (y, yp), call again.
 * Profiles are scalars or samples on the model grid zg (np.interp'ed on the device).      */
#define PM_EQ_HFREE 1       /* H is an unknown parameter (p in/out), else p = H fixed      */
#define PM_EQ_HAS_BBOT 2    /* bottom condition d2Psi(-1) = b_bot/H, else d3Psi(-1) = -bz(H) */
#define PM_EQ_KAPPA_ARRAY 4 /* kappa_z / dkappa_z tables are used instead of the scalar kappa */
#define PM_EQ_PSI_ARRAY 8   /* psi_z table is used (otherwise psi_so = 0)                  */
typedef struct pm_equi_column {
  int32_t n, nzg, mmax, reserved;
  const int32_t *m;       /* [n] mesh nodes of each member, 3 <= m <= mmax                */
  const int32_t *active;  /* [n] 0 = skip this member (may be NULL)                       */
  const double *x;        /* [n][mmax] mesh on [-1, 0]                                    */
  double *y;              /* [n][4][mmax] in: initial guess; out: final Newton iterate    */
  double *yp;             /* [n][4][mmax] out: ode(x, y) at the nodes (spline derivatives) */
  double *p;              /* [n] in/out: H (initial guess -> solution with PM_EQ_HFREE)   */
  const double *f;        /* [n] Coriolis parameter                                       */
  const double *A;        /* [n] basin area                                               */
  const double *bs;       /* [n] -b_s/f^2  (Equi_Column.bs)                               */
  const double *bb;       /* [n] -b_bot/f^2 (Equi_Column.b_bot) with PM_EQ_HAS_BBOT, else B_int */
  const double *kappa;    /* [n] scalar diffusivity (ignored with PM_EQ_KAPPA_ARRAY)      */
  const int32_t *flags;   /* [n] PM_EQ_* */
  const double *zg;       /* [nzg] the model's z grid for array profiles (NULL if unused) */
  const double *kappa_z;  /* [n][nzg] kappa on zg                                         */
  const double *dkappa_z; /* [n][nzg] np.gradient(kappa, zg)                              */
  const double *psi_z;    /* [n][nzg] psi_so on zg                                        */
  double tol;             /* solve_bvp's tol = bc_tol (the reference uses the default 1e-3) */
  double *rms;            /* [n][mmax] out: rms residual of every interval (may be NULL)  */
  int32_t *nadd;          /* [n] out: nodes solve_bvp would insert (may be NULL)          */
  int32_t *status;        /* [n] out: 2 = singular Jacobian, else 0 (may be NULL)         */
  int32_t *niter;         /* [n] out: Newton iterations taken (may be NULL)               */
  double *info;           /* [n][2] out: max rms residual, max |bc residual| (may be NULL) */
  double *scratch;        /* [n][pm_equi_column_scratch_doubles(mmax)] workspace          */
} pm_equi_column;

size_t pm_equi_column_scratch_doubles(int32_t mmax);
int pm_equi_column_newton(const pm_equi_column *eq, pm_stream_t stream);

/* out[i] = alpha*x[i] + beta*y[i] (two products, one sum, in that order): the relaxation
 * b1 <- 0.8*b1 + 0.2*basin.b of examples/example_iteration.py:67.                         */
int pm_axpby(size_t count, double alpha, const double *x, double beta, const double *y,
             double *out, pm_stream_t stream);

/* ------------------------------------------------------------------ RCCL
 * One process per GPU.  The ensemble is sharded by member, stepping needs no
 * communication; the only exchange is the gather of per-member output at diagnostic
 * time (the reference has no distributed path: SURVEY.md section 5/8e).  librccl.so is
 * dlopen()ed on first use, so single-GPU runs never load it.
 * Bootstrap: rank 0 calls pm_comm_unique_id and ships the 128 bytes to the other ranks
 * by any host channel; then every rank calls pm_comm_init.                          */
#define PM_COMM_ID_BYTES 128
int pm_comm_unique_id(void *id128);
int pm_comm_init(pm_comm_t *comm, int32_t nranks, int32_t rank, const void *id128);
int pm_comm_destroy(pm_comm_t comm);
/* recv[nranks][count] <- send[count] of every rank (fp64, device pointers) */
int pm_comm_allgather(pm_comm_t comm, const void *send, void *recv, size_t count,
                      pm_stream_t stream);
/* gather to ONE rank: recv[nranks][count] on `root` <- send[count] of every rank (point-to-point
 * ncclSend / ncclRecv in one group; the root's own block is a device copy).  `recv` is only
 * read on the root and may be NULL elsewhere.  The diagnostic exchange needs no more than this:
 * one process writes the output (the reference's script is that process).  With nranks = 1 the
 * root sends to itself through RCCL when `self_loop` != 0 (plumbing rehearsal), else copies.   */
int pm_comm_gather_root(pm_comm_t comm, const void *send, void *recv, size_t count, int32_t root,
                        int32_t self_loop, pm_stream_t stream);
/* elementwise max over ranks (fp64, device pointers; in place allowed) */
int pm_comm_allreduce_max(pm_comm_t comm, const void *send, void *recv, size_t count,
                          pm_stream_t stream);
/* all ranks have reached this point AND their `stream` work before it is done */
int pm_comm_barrier(pm_comm_t comm, pm_stream_t stream);

/* debug/test: the kernels' two divisions by a precomputed reciprocal (div_by_recip from RN(1/d),
 * div_by_recip2 from the double-double reciprocal; both must be correctly rounded) against IEEE `/` on
 * `4*per_thread*256*blocks` random operand pairs (exponents within +-emax, 3/8 of the
 * mantissas at the all-ones / all-zeros / half-way edges); bitwise mismatches counted. */
int pm_selftest_fastdiv(uint64_t seed, int32_t blocks, int32_t per_thread, int32_t emax,
                        uint64_t *tested, uint64_t *mismatches);

/* Host function (no device work): *proven = 1 when, for EVERY one of the n denominators, the
 * 3-instruction quotient  y = RN(1/d); q0 = RN(a y); r = fma(-d, q0, a); q = fma(r, y, q0)  is the
 * correctly rounded a / d for every numerator a (finite operands whose quotient and residual stay
 * normal).  Only numerators whose quotient lies within 3 * 2^-53 ulp of a rounding boundary could
 * fail; for a given d they are the <= ~12 solutions of a congruence on the integer mantissas,
 * which the function enumerates and runs through the very sequence (div_proof.h: div3_proof).
 * Zero, subnormal and non-finite denominators are "not proven".  `candidates` (may be NULL)
 * receives the number of numerators tested.  What a caller establishes before it sets
 * PM_COLS_DIV3_PROVEN.  Replaces nothing of the reference (which divides in NumPy); it licenses
 * a cheaper instruction sequence for column.py:235-247's three divisions.                       */
int pm_div3_proven(const double *d, int64_t n, int32_t *proven, int64_t *candidates);

/* The proof above takes y = RN(1/d); the kernels form y on the DEVICE, whose fp64 `/` is not
 * correctly rounded in every case (see pm_selftest_div3).  *ok = 1 when the device's 1.0 / d[i]
 * equals the host's IEEE quotient bit for bit for all n host-side denominators (one small launch;
 * the kernels' prologues evaluate the same expression).  A caller sets PM_COLS_DIV3_PROVEN only
 * when both pm_div3_proven and pm_recip_check hold for the batch's denominators.               */
int pm_recip_check(const double *d, int64_t n, int32_t *ok);

/* Host function (no device work): proven[i] = 1 when the 2-instruction quotient
 *   yh = RN(1/d); yl = RN((1 - d yh) / d); q = fma(a, yh, RN(a yl))
 * is the correctly rounded a / d[i] for every numerator a (same operand window as above).  The last
 * fma rounds (a/d)(1 + eta) with |eta| < 2.01 * 2^-106, so only numerators whose quotient lies within
 * 4 / (2 D) ulp of a rounding midpoint could fail (D: d's 53-bit integer mantissa); they are
 * enumerated as in pm_div3_proven and run through the very sequence (div_proof.h: div2_proof).
 * There is no correction step, so some denominators DO fail (about 1 % of arbitrary mantissas; none
 * whose mantissa has three or more trailing zero bits, which have no candidate at all): the verdict is
 * per denominator.  `candidates` (may be NULL) receives the number of numerators tested.  What a
 * caller establishes before it sets PM_COLS_DIV2_GRID / PM_COL_DIV2_AREA.                        */
int pm_div2_proven(const double *d, int64_t n, int32_t *proven /* [n] */, int64_t *candidates);

/* pm_recip_check's sibling for that form: ok[i] = 1 when the device's yh = 1.0 / d[i] AND its low part
 * yl = fma(-d[i], yh, 1.0) / d[i] equal the host's bit for bit (one small launch; the kernel's
 * prologue evaluates the same expressions).  pm_div2_proven's verdict is valid for that pair only. */
int pm_recip2_check(const double *d, int64_t n, int32_t *ok /* [n] */);

/* debug/test: the DEVICE's 2-instruction quotient against the HOST's IEEE `/` on the candidate
 * numerators of `ndenoms` random denominators (drawn as in pm_selftest_div3; numerators of both
 * signs, rescaled) plus two arbitrary numerators for each proven one.  `mismatches` counts the pairs
 * whose denominator pm_div2_proven accepts and must be 0; `unproven` = denominators the proof
 * rejected, `unproven_mismatches` the differing pairs among THEIR candidates (not zero: that is why
 * they are rejected).                                                                            */
int pm_selftest_div2(uint64_t seed, int32_t ndenoms, uint64_t *tested, uint64_t *mismatches,
                     uint64_t *unproven, uint64_t *unproven_mismatches);

/* debug/test: the DEVICE's 3-instruction quotient against the HOST's IEEE `/` on the candidate
 * numerators of `ndenoms` random denominators (uniform mantissas, mantissas next to 1 and 2,
 * mantissas with trailing zeros; numerators of both signs, rescaled) plus two arbitrary numerators
 * each: `mismatches` must be 0.  `unproven` = denominators the host proof rejected (their
 * candidates are tested all the same).  `device_div_off` = pairs on which the device's own
 * `a / d` differs from the host's quotient: NOT zero on gfx950 -- about 1e-4 of these
 * near-midpoint quotients come out one ulp off (its final correction does not use a correctly
 * rounded reciprocal); for an arbitrary operand pair that is a ~1e-19 event.                    */
int pm_selftest_div3(uint64_t seed, int32_t ndenoms, uint64_t *tested, uint64_t *mismatches,
                     uint64_t *unproven, uint64_t *device_div_off,
                     double *one_bad_pair /* {a, d} of a mismatch, or NULL */);

/* debug/test: the wave scans of the GM boundary-value solve (DPP row steps + row joins: element
 * prefix / suffix scans, the affine suffix scan, the node-count prefix sum) against the same
 * compositions done serially, for `nhas` (1..64) occupied lanes: max_rel3 = largest relative
 * deviations {prefix, suffix, affine} (association differs: ~1e-14), sum_mismatches = lanes whose
 * integer prefix sum differs (must be 0). */
int pm_selftest_so_scans(int32_t nhas, uint64_t seed, double *max_rel3, int32_t *sum_mismatches);

/* debug/test: lane-shift primitive self check (DPP wave shifts vs ds_bpermute) */
int pm_selftest_lane_shift(int32_t *mismatches);

/* ------------------------------------------------------------------ sections
 * pymoc.plotting's section interpolators, every member of an ensemble at once:
 *   PM_SEC_CHANNEL  Interpolate_channel.__call__ (src/pymoc/plotting/interp_channel.py:40-62):
 *                   bs on y, bn on z, isopycnals of constant slope from the channel surface;
 *   PM_SEC_TWOCOL   Interpolate_twocol.__call__ (src/pymoc/plotting/interp_twocol.py:37-73):
 *                   bs and bn on z, isopycnals between the two columns;
 * evaluated on the query grid yq x zq as gridit does (src/pymoc/utils/gridit.py:24-30:
 * out[m][i][j] = f(yq[i], zq[j])).  Profiles are np.interp'ed (make_func, utils/make_func.py:31-44)
 * unless PM_SEC_BS_SCALAR / PM_SEC_BN_SCALAR make them a float (value + 0*x).  The root finds are
 * scipy.optimize.brenth with SciPy 1.15.3's defaults (xtol 2e-12, rtol 4 eps, maxiter 100,
 * scipy/optimize/Zeros/brenth.c) in the same IEEE fp64 operations, so a finite section is
 * bit-identical to the reference's.  Where brenth raises, the point is NaN and its status says
 * why: PM_SEC_ESIGN "f(a) and f(b) must have different signs" (ValueError), PM_SEC_ECONV
 * "Failed to converge after 100 iterations." (RuntimeError), PM_SEC_ENAN the function value is
 * NaN (SciPy's ValueError guard, optimize/_zeros_py.py:_wrap_nan_raise).
 * Member m's bs row is bs[bs_offset + m * bs_stride ...] (in doubles), so rows of an ensemble's
 * state (ColumnBatch.b, SOMLBatch.bs) are read in place; stride 0 shares one row.
 * Fix-ups (applied to the member's LDS copy, never to the input):
 *   PM_SEC_FIX_PLOT_OVERTURNING  channel: Plot_overturning.py:42-50 (bs[0] = bs[1] if bs[0] > bs[1],
 *                                then bn[0] = bs[0] if bs[0] < bn[0]); twocol: :63-64 (bn[0] = bs[0])
 *   PM_SEC_FIX_TWOBASIN          channel only: twobasin_NadeauJansen.py:176 (bs[-1] = bn[-1])
 * Sizes: 2 <= ny, nz <= 1024 (the member's profiles and axes are staged in LDS), 1 <= nyq, nzq
 * <= 1024.  y, z sorted ascending (as np.interp requires).                                  */
#define PM_SEC_CHANNEL 0
#define PM_SEC_TWOCOL 1
#define PM_SEC_BS_SCALAR 1            /* flags: bs is a float per member (bs_len ignored)   */
#define PM_SEC_BN_SCALAR 2            /* flags: bn is a float per member                    */
#define PM_SEC_FIX_PLOT_OVERTURNING 1 /* fixups */
#define PM_SEC_FIX_TWOBASIN 2
#define PM_SEC_OK 0
#define PM_SEC_ESIGN 1
#define PM_SEC_ECONV 2
#define PM_SEC_ENAN 3
#define PM_SEC_MAX_LEVELS 1024
typedef struct pm_sections {
  int32_t n, kind, ny, nz;      /* members, PM_SEC_*, profile axes y[ny], z[nz]              */
  int32_t nyq, nzq, flags, fixups;
  const double *y, *z;          /* [ny], [nz] the classes' grids (l = y[ny-1], z[0] = bottom) */
  const double *yq, *zq;        /* [nyq], [nzq] query grid                                   */
  const double *bs;             /* channel: [ny] per member, twocol: [nz] per member          */
  int64_t bs_offset, bs_stride; /* in doubles */
  const double *bn;             /* [nz] per member                                           */
  int64_t bn_offset, bn_stride;
  double *out;                  /* [n][nyq][nzq] out: the section, NaN where brenth raised   */
  uint8_t *status;              /* [n][nyq][nzq] out: PM_SEC_OK / ESIGN / ECONV / ENAN (or NULL) */
  int32_t *first;               /* [n] out: first failing point i*nzq + j in gridit order, -1 none (or NULL) */
} pm_sections;

int pm_sections_grid(const pm_sections *sec, pm_stream_t stream);

/* ------------------------------------------------------------------ overturning sections
 * The three fields the reference's figure script plots, examples/Plot_overturning.py:73-92, for
 * every member of an ensemble: the depth-space (psi_z), isopycnal (psi_b) and residual (psi_res)
 * overturning on the section [nrows][nz] assembled from the channel (ny rows), the basin (n_basin
 * rows, every one the basin profile) and the north (n_north rows), nrows = ny + n_basin + n_north:
 *   row 0                 zero in all three fields (the script's loop starts at 1)
 *   channel rows >= 1     psi_res = psi_z = np.interp(bnew[iy], b_basin, Psi_SO)           (:79-80)
 *                         psi_b[k] = Psi_SO[k] where b_basin[k] < bs_SO[iy], else 0        (:81)
 *   basin rows            psi_res = psi_b = (c1[iy]*psibz1 + c2[iy]*Psi_SO)/lbasin         (:84, :86)
 *                         psi_z = (c1[iy]*Psi + c2[iy]*Psi_SO)/lbasin                      (:85)
 *   north rows            psi_res = np.interp(bnew[iy], bgrid, psib)                       (:89)
 *                         psi_z = (c3[iy]*Psi)/lnorth                                      (:90)
 *                         psi_b[k] = psibz1[k] where b_basin[k] < bnew[iy][nz-1], else 0   (:91)
 *   last row              psi_res = 0                                                      (:92)
 * bnew = concatenate(bsouth, tile(b_basin), bnorth) (:71).  c1 = ynew - lchannel, c2 = lchannel +
 * lbasin - ynew, c3 = lchannel + lbasin + lnorth - ynew are formed by the caller in the script's
 * order (the row coordinate ynew itself is not needed here); a comparison with NaN is false.
 * IEEE fp64 in the script's operation order, np.interp as in pm_sections_grid: bit-identical.
 * Member m's row of an input starts `offset + m * stride` doubles into it (pm_rows), so rows of an
 * ensemble's state and of the solvers' outputs are read in place; stride 0 shares one row.
 * Per member and field the maximum and minimum over the section with the row-major index
 * iy*nz + k of their first occurrence (np.argmax / np.argmin); a field that holds a NaN reports NaN
 * and the first NaN's index for both.  Fields: PM_OVT_Z, PM_OVT_B, PM_OVT_RES.
 * status bits: PM_OVT_NAN_SECTION bnew holds a NaN (a point where the reference's brenth raises:
 * the script would have stopped), PM_OVT_BAD_BASIN b_basin is non-finite or not non-decreasing
 * (np.interp's result then depends on its search order); such members get whatever the
 * interpolation gives and do not disturb the others.
 * Sizes: 2 <= nz, ny <= 1024, 1 <= nb <= 2048, n_basin, n_north >= 1, n_basin + n_north <= 1024.  */
#define PM_OVT_Z 0
#define PM_OVT_B 1
#define PM_OVT_RES 2
#define PM_OVT_NAN_SECTION 1
#define PM_OVT_BAD_BASIN 2
#define PM_OVT_MAX_LEVELS 1024
#define PM_OVT_MAX_NB 2048
typedef struct pm_rows {
  const double *ptr;
  int64_t offset, stride;     /* in doubles */
} pm_rows;
typedef struct pm_overturning {
  int32_t n, nz, ny, nb;      /* members, levels, channel rows, isopycnal classes            */
  int32_t n_basin, n_north;   /* basin and north rows (the script: 60 and 10)                */
  int32_t reserved1, reserved2;
  pm_rows b_basin;            /* [nz] raw basin buoyancy                                     */
  pm_rows bs_SO;              /* [ny] raw channel surface buoyancy                           */
  pm_rows Psi;                /* [nz] AMOC.Psi                                               */
  pm_rows Psi_SO;             /* [nz] PsiSO.Psi                                              */
  pm_rows bgrid;              /* [nb] AMOC.bgrid                                             */
  pm_rows psib;               /* [nb] AMOC.Psib(nb)                                          */
  pm_rows psibz1;             /* [nz] AMOC.Psibz(nb)[0]                                      */
  pm_rows bsouth;             /* [ny][nz] channel section                                    */
  pm_rows bnorth;             /* [n_north][nz] northern section                              */
  const double *c1, *c2, *c3; /* [nrows] shared row coefficients                             */
  double lbasin, lnorth;
  double *psi_z, *psi_b, *psi_res; /* [n][nrows][nz] out, each may be NULL (not stored)      */
  double *bnew;               /* [n][nrows][nz] out: the assembled section (may be NULL)     */
  double *extrema;            /* [n][3][2] out: {max, min} of PM_OVT_Z / _B / _RES (may be NULL) */
  int32_t *extrema_at;        /* [n][3][2] out: their indices iy*nz + k (may be NULL)        */
  int32_t *status;            /* [n] out: PM_OVT_* bits (may be NULL)                        */
} pm_overturning;

int pm_overturning_sections(const pm_overturning *d, pm_stream_t stream);

/* ------------------------------------------------------- two-basin overturning sections
 * What examples/twobasin_NadeauJansen.py builds after its loop (:157-262), for every member of an
 * ensemble: eight overturning fields and three buoyancy sections on the section [nrows][nz] of
 * channel (ny rows), basin (n_basin), northern transition (n_trans) and northern sinking region
 * (n_north), nrows = ny + n_basin + n_trans + n_north (the script: 51 + 60 + 20 + 20).
 *
 * pm_twobasin_profiles (:161, :192-193) -- the two derived rows the section interpolators need:
 *   b_basin = (A_Atl*b_Atl + A_Pac*b_Pac)/(A_Atl + A_Pac)          A_* one double per member
 *   bn      = b_north with bn[0] = b_basin[0]
 *
 * pm_twobasin_overturning_sections (:166-168, :203-262).  Per member, once:
 *   b_basin as above;  sum = Psi_SO_Atl + Psi_SO_Pac;  iA = np.interp(b_basin, b_Atl, Psi_SO_Atl),
 *   iP = np.interp(b_basin, b_Pac, Psi_SO_Pac), PsiSO = iA + iP                        (:166-167)
 *   Ab = np.interp(b_basin, bgrid_AMOC, psib_AMOC)                                     (:168)
 *   Zb = np.interp(b_basin, bgrid_ZOC, psib_ZOC)                                       (:236, :239)
 * then with x = bnew[iy] (the row of the assembled section), c1..c3 the row coefficients:
 *   row 0            zero in all eight fields (the script's loop starts at 1)
 *   channel, >= 1    Z = Z_ATL = Z_PAC = np.interp(x, b_basin, sum)                    (:218-220)
 *                    B = B_ATL = B_PAC = PsiSO[k] where b_basin[k] < bs_SO[iy], else 0 (:221-225)
 *                    ATL = PAC = np.interp(x, b_basin, PsiSO)                          (:222, :224)
 *   basin            Z     = (c1*Psi_AMOC + c2*sum)/lbasin                             (:228)
 *                    Z_ATL = (c1*Psi_AMOC + c2*(Psi_SO_Atl - Psi_ZOC))/lbasin          (:229)
 *                    Z_PAC = (c2*(Psi_SO_Pac + Psi_ZOC))/lbasin                        (:230)
 *                    B     = (c1*Ab + c2*PsiSO)/lbasin                                 (:231-232)
 *                    ATL   = (c1*psibz_AMOC1 + c2*(Psi_SO_Atl - psibz_ZOC1))/lbasin    (:233)
 *                    B_ATL = (c1*Ab + c2*(iA - Zb))/lbasin                             (:234-236)
 *                    PAC   = (c2*(Psi_SO_Pac + psibz_ZOC2))/lbasin                     (:237)
 *                    B_PAC = (c2*(iP + Zb))/lbasin                                     (:238-239)
 *   transition       Z = Z_ATL = Psi_AMOC;  ATL = np.interp(x, bgrid_AMOC, psib_AMOC)  (:244-248)
 *                    B = B_ATL = Ab[k] where b_basin[k] < x[nz-1], else 0              (:247, :249)
 *   north            Z = Z_ATL = (c3*Psi_AMOC)/lnorth;  ATL = (c3*psibz_AMOC2)/lnorth  (:254-259)
 *                    B = B_ATL = (c3*Ab[k])/lnorth where b_basin[k] < x[nz-1], else 0  (:257-260)
 *   transition and north: Z_PAC = B_PAC = PAC = NaN                                    (:246-262)
 * The last row is NOT zeroed (Plot_overturning.py does that, this script does not).
 *   bnew     = concatenate(bsouth, tile(b_basin), btrans, tile(bn))                    (:203)
 *   bnew_Atl = ... tile(b_Atl) in the basin rows                                       (:204)
 *   bnew_Pac = ... tile(b_Pac) in the basin rows, NaN in transition and north          (:205)
 * c1 = ynew - lchannel, c2 = lchannel + lbasin - ynew, c3 = lchannel + lbasin + ltrans + lnorth -
 * ynew are formed by the caller in the script's order.  IEEE fp64 in the script's operation order,
 * `/` for its divisions, np.interp as in pm_sections_grid: bit-identical.  Inputs are pm_rows as
 * for pm_overturning; one nb serves both thermal winds (the script: 500 for both).
 * Every output may be NULL (not stored); extrema and status are computed regardless.
 * extrema [n][8][2] = {max, min} per field, extrema_at their indices iy*nz + k, with the contract
 * of pm_overturning (first occurrence; a NaN gives NaN and the first NaN's index); the three
 * Pacific fields over the rows the script defines, field[:ny + n_basin].
 * status bits: PM_TBO_NAN_SECTION a NaN in bsouth / btrans / bn; PM_TBO_BAD_BASIN / _BAD_ATL /
 * _BAD_PAC b_basin / b_Atl / b_Pac non-finite or not non-decreasing; PM_TBO_BAD_BGRID_AMOC / _ZOC
 * that bgrid not non-decreasing.  Such a member gets whatever the interpolation gives and does not
 * disturb the others.
 * Sizes: 2 <= nz, ny <= 1024, 1 <= nb <= 2048, n_basin, n_trans, n_north >= 1 and together <=
 * 1024, and the member's rows must fit one workgroup's LDS: pm_twobasin_overturning_lds_bytes
 * (17 rows of nz, one of ny, two of nb doubles, each padded to 16 bytes, plus the reduction's
 * scratch) <= 160 KB -- nz = ny = 512 with nb = 2048 is 105 KB and runs, nz = 1024 with nb = 2048
 * (177 KB) does not.  PM_EINVAL beyond.                                                       */
#define PM_TBO_Z 0
#define PM_TBO_Z_ATL 1
#define PM_TBO_Z_PAC 2
#define PM_TBO_B 3
#define PM_TBO_B_ATL 4
#define PM_TBO_B_PAC 5
#define PM_TBO_ATL 6
#define PM_TBO_PAC 7
#define PM_TBO_FIELDS 8
#define PM_TBO_NAN_SECTION 1
#define PM_TBO_BAD_BASIN 2
#define PM_TBO_BAD_ATL 4
#define PM_TBO_BAD_PAC 8
#define PM_TBO_BAD_BGRID_AMOC 16
#define PM_TBO_BAD_BGRID_ZOC 32
#define PM_TBO_MAX_LEVELS 1024
#define PM_TBO_MAX_NB 2048
typedef struct pm_twobasin_rows {
  int32_t n, nz;
  pm_rows b_Atl, b_Pac, b_north; /* [nz] the three columns                                   */
  pm_rows A_Atl, A_Pac;          /* [1] the basins' areas, per member                        */
  double *b_basin, *bn;          /* [n][nz] out                                              */
} pm_twobasin_rows;
typedef struct pm_twobasin_overturning {
  int32_t n, nz, ny, nb;         /* members, levels, channel rows, isopycnal classes         */
  int32_t n_basin, n_trans, n_north; /* the script: 60, 20, 20                               */
  int32_t reserved;
  pm_rows b_Atl, b_Pac;          /* [nz] Atl.b, Pac.b                                        */
  pm_rows A_Atl, A_Pac;          /* [1]                                                      */
  pm_rows bs_SO;                 /* [ny] raw channel surface buoyancy                        */
  pm_rows Psi_SO_Atl, Psi_SO_Pac, Psi_AMOC, Psi_ZOC;              /* [nz]                    */
  pm_rows psibz_AMOC1, psibz_AMOC2; /* [nz] AMOC.Psibz(nb)[0], [1]                           */
  pm_rows psibz_ZOC1, psibz_ZOC2;   /* [nz] ZOC.Psibz()[0], [1]                              */
  pm_rows bgrid_AMOC, psib_AMOC, bgrid_ZOC, psib_ZOC;             /* [nb]                    */
  pm_rows bsouth;                /* [ny][nz] channel section                                 */
  pm_rows btrans;                /* [n_trans][nz] transition section                         */
  pm_rows bn;                    /* [nz] pm_twobasin_profiles' bn                            */
  const double *c1, *c2, *c3;    /* [nrows] shared row coefficients                          */
  double lbasin, lnorth;
  double *psi[PM_TBO_FIELDS];    /* [n][nrows][nz] out, each may be NULL (not stored)        */
  double *bnew, *bnew_Atl, *bnew_Pac; /* [n][nrows][nz] out, each may be NULL                */
  double *extrema;               /* [n][8][2] out: {max, min} per field (may be NULL)        */
  int32_t *extrema_at;           /* [n][8][2] out: their indices iy*nz + k (may be NULL)     */
  int32_t *status;               /* [n] out: PM_TBO_* bits (may be NULL)                     */
} pm_twobasin_overturning;

int pm_twobasin_profiles(const pm_twobasin_rows *d, pm_stream_t stream);
int pm_twobasin_overturning_lds_bytes(int32_t nz, int32_t ny, int32_t nb, size_t *bytes);
int pm_twobasin_overturning_sections(const pm_twobasin_overturning *d, pm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Convergence check of an ensemble run to steady state (pymoc_amd.run_to_steady), ONE launch
 * over the n rows of the current batch.  Row m holds original member k = orig[m]; rows whose
 * member is no longer PM_STEADY_RUNNING are not touched.  For a running member:
 *   d = max over the drift fields f and levels i of |src_f[m][i] - buf_f[m][i]|  (fmax: exact,
 *       independent of order -- bitwise np.max(np.abs(cur - ref)) * scale);
 *   drift_out[k] = d * scale (NaN when an element of src or snapshot is non-finite), then the
 *       snapshot row buf_f[m] = src_f[m];
 *   non-finite element -> PM_STEADY_NONFINITE; else streak[k] = (d * scale <= tol[k]) ?
 *       streak[k] + 1 : 0, PM_STEADY_CONVERGED when streak[k] >= consecutive; else with
 *       `finalize` PM_STEADY_MAXSTEPS;
 *   a member that retires here has every capture field's src row copied to buf_c[k] and
 *       step_out[k] = step;
 *   members still running are counted into *n_running (zeroed by this entry first).
 * Sizes: 0 <= n <= n0, 1 <= ndrift <= 4, 0 <= ncapture <= 8, consecutive >= 1, every field
 * len >= 1 and src_stride >= len (doubles).                                                   */
#define PM_STEADY_RUNNING 0
#define PM_STEADY_CONVERGED 1
#define PM_STEADY_NONFINITE 2
#define PM_STEADY_MAXSTEPS 3
#define PM_STEADY_MAX_DRIFT 4
#define PM_STEADY_MAX_CAPTURE 8
typedef struct pm_steady_field {
  const double *src; int64_t src_stride; /* row m of the live state at src + m*src_stride        */
  double *buf;                           /* drift field: snapshot [n][len]; capture: result [n0][len] */
  int32_t len, reserved;
} pm_steady_field;
struct pm_steady_check {
  int32_t n, n0, ndrift, ncapture;       /* rows now, members at the start, <=4 drift, <=8 capture */
  int32_t consecutive, finalize;
  int64_t step;                          /* steps taken at this check                             */
  double scale;                          /* drift = scale * max |src - snapshot|                   */
  const int32_t *orig;                   /* [n]  original member of row m                          */
  const double *tol;                     /* [n0] per member                                        */
  int32_t *streak, *status;              /* [n0] in/out                                            */
  double *drift_out; int64_t *step_out;  /* [n0]                                                   */
  int32_t *n_running;                    /* [1]  out, zeroed by the entry before the launch        */
  pm_steady_field drift[PM_STEADY_MAX_DRIFT], capture[PM_STEADY_MAX_CAPTURE];
};
/* the struct is named by its tag only: a typedef of the same name would clash with the function */
int pm_steady_check(const struct pm_steady_check *c, pm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Time-dependent forcing of an ensemble (pymoc_amd.ForcingSchedule), ONE launch: a piecewise-
 * linear schedule evaluated at time t and written into up to 8 target arrays that the stepping
 * kernels re-read at every launch (the columns' bs, the channel's tau, bs_SO, b_rest, surflux).
 * (no counterpart: the user loop's assignments `basin.bs = ...`, `PsiSO.tau = ...` ahead of a
 * step.)
 *   knots   [K] HOST array, strictly increasing and finite, shared by all members and targets:
 *           the bracket of t depends on t alone, so the entry finds it here, once, and the kernel
 *           receives it as arguments;
 *   target  rows [row0, row0 + n) of a dense array of rows of `len` doubles at `dst` (`bs_north`
 *           is rows [n, 2n) of the columns' bs with len = 1); `values` holds the knot values,
 *           knot axis first: [K][len] shared by all members (per_member = 0) or [K][n][len]
 *           (per_member = 1: one knot's slab is the target's own layout, so its loads coalesce
 *           across members and levels exactly as the stores do).
 * Every written element equals np.interp(t, knots, values of that element) BIT FOR BIT: values
 * held outside the knots, the value itself on a knot, K = 1, slope = (f1 - f0) / (x1 - x0) then
 * slope * (t - x0) + f0 uncontracted, np.interp's fallbacks when that is NaN; t = NaN writes NaN
 * (with K = 1 the knot's value, as np.interp does).
 * Nothing outside the n rows of a target is touched.
 * Sizes: n >= 1, K >= 1, 1 <= ntargets <= 8, every len >= 1 and row0 >= 0, no NULL pointer.     */
#define PM_FORCING_MAX_TARGETS 8
typedef struct pm_forcing_target {
  double *dst; int64_t row0;             /* rows [row0, row0 + n) of [.][len] are written         */
  const double *values;                  /* device: [K][len] or [K][n][len]                       */
  int32_t len, per_member;
} pm_forcing_target;
struct pm_forcing {
  int32_t n, K, ntargets, reserved;
  const double *knots;                   /* HOST [K]                                              */
  pm_forcing_target target[PM_FORCING_MAX_TARGETS];
};
/* the struct is named by its tag only, as pm_steady_check's is */
int pm_forcing_apply(const struct pm_forcing *f, double t, pm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Per-member indices of rows (pymoc_amd.RowIndices / IndexRecorder), ONE launch: up to
 * PM_INDICES_MAX specifications evaluated for every member, written as
 *   value[s][m] (fp64) and pos[s][m] (int32),  s < nspec, m < n
 * at the caller's addresses -- a recorder passes record k of its device series, so a sample is
 * this launch alone.  (no counterpart: what a user computes from the profiles after the loop,
 * `np.max(AMOC.Psi)`, `z[np.argmax(AMOC.Psi)]`, `np.interp(-1000., z, basin.b)`.)
 *   spec      HOST copy of the table: every call checks it;
 *   spec_dev  the same nspec entries in DEVICE memory, uploaded once by the table's owner: the
 *             kernel walks the table in memory (as a kernel argument indexed at run time it would
 *             be copied to scratch).
 * An entry names rows `stride` doubles apart (row m of the source at src + m * stride: the drivers'
 * fields are row views into stacked arrays), their length nlev, the axis of the levels (device,
 * nlev doubles), the inclusive window lo..hi of levels and one parameter.  With r = row[lo..hi]:
 *   PM_IDX_MAX    value = row[pos], the very bits; pos = lo + np.argmax(r): first occurrence, a
 *                 NaN wins, the first NaN
 *   PM_IDX_MIN    value = row[pos]; pos = lo + np.argmin(r)
 *   PM_IDX_AT     value = np.interp(param, axis, row) over the WHOLE row (lo, hi unused), bit for
 *                 bit, for a strictly increasing axis; pos = -1
 *   PM_IDX_CROSS  the level c = param: if row[hi] == c: value = axis[hi], pos = hi.  Otherwise
 *                 pos = the largest i in [lo, hi - 1] with (row[i] - c <= 0 < row[i+1] - c) or
 *                 (row[i] - c >= 0 > row[i+1] - c), t = (c - row[i]) / (row[i+1] - row[i]) and
 *                 value = axis[i] + t * (axis[i+1] - axis[i]), uncontracted.  No such i: NaN, -1
 *   PM_IDX_MEAN   value = S / (axis[hi] - axis[lo]), S = sum over i in [lo, hi - 1] of
 *                 0.5 * (row[i] + row[i+1]) * (axis[i+1] - axis[i]); hi == lo: row[lo]; pos = -1.
 *                 The summation order is the kernel's own: the one index that is a tolerance path.
 * Checked before anything is launched (PM_EINVAL, outputs untouched): n >= 1, 1 <= nspec <=
 * PM_INDICES_MAX, nlev >= 1, 0 <= lo <= hi < nlev, stride >= nlev, no NULL pointer, kind known.
 * That rows [0, n) of every source lie inside its allocation is the caller's to ensure.         */
#define PM_INDICES_MAX 32
#define PM_IDX_MAX 0
#define PM_IDX_MIN 1
#define PM_IDX_AT 2
#define PM_IDX_CROSS 3
#define PM_IDX_MEAN 4
typedef struct pm_index_spec {
  const double *src;                     /* device: row m at src + m * stride                     */
  const double *axis;                    /* device [nlev]                                         */
  int64_t stride;                        /* doubles between rows, >= nlev                         */
  int32_t nlev, kind, lo, hi;
  double param;                          /* PM_IDX_AT: x0; PM_IDX_CROSS: the level                */
} pm_index_spec;
struct pm_row_indices {
  int32_t n, nspec;
  const pm_index_spec *spec;             /* HOST [nspec]                                          */
  const pm_index_spec *spec_dev;         /* DEVICE [nspec], the same entries                      */
};
/* the struct is named by its tag only, as pm_steady_check's is */
int pm_row_indices(const struct pm_row_indices *d, double *value, int32_t *pos,
                   pm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Stochastic forcing of an ensemble (pymoc_amd.NoiseForcing), ONE launch per application: every
 * member's red-noise state advances by one Gaussian deviate generated on the device, and
 * base + state * pattern is written into up to 8 destination arrays -- the arrays
 * pm_forcing_apply writes.  (no counterpart: an extension.)
 *
 * Deviate xi(seed, id, j, stream): Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl
 * constants 0x9E3779B9 / 0xBB67AE85) with
 *   key     = { seed & 0xffffffff, seed >> 32 }
 *   counter = { id & 0xffffffff, id >> 32, j, stream },  id = member0 + m
 * (j: the application index the caller counts; stream: the target's position in
 * bs, bs_north, tau, b_rest, surflux, bs_SO).  From the four output words r0..r3, in fp64:
 *   d1 = ((r0 >> 5) * 67108864.0 + (r1 >> 6)) * 2^-53,  d2 likewise from r2, r3   (exact)
 *   R  = sqrt(-2.0 * log(1.0 - d1))
 *   xi = R * cos(6.283185307179586 * d2)
 * uncontracted, in this order: d1, d2, 1.0 - d1 (in [2^-53, 1]) and the cosine's argument are
 * exact-arithmetic results; only log and cos are the device library's (a tolerance against a host
 * restatement: |xi - xi_host| <= 16 * 2^-53 * R).  A deviate depends on nothing but its four
 * coordinates: not on n, on the shard, or on which other targets a launch perturbs.
 * State, per target and member:  x_out[m] = a * x_in[m] + (sigma[m] * b) * xi, uncontracted; a
 * and b are the caller's (a = exp(-dt / tau_corr), b = sqrt(1 - a * a); a = 0, b = 1 for white
 * noise and for the first application on a zeroed state).  Every thread of member m recomputes
 * x_out[m] from x_in[m]; the thread of element 0 stores it -- into the OTHER buffer, which the
 * caller swaps with x_in between applications, so no launch reads what it writes.
 * Value:  dst[row0 + m][i] = base[m][i] + x_out[m] * pattern[i], uncontracted (pattern [len], or
 * [n][len] with pattern_per_member = 1; NULL: base + x_out).
 * Entries that name the same quantity kept in two places share one state: the same `stream` and
 * x_in give them the same x_out value; x_out and xi_out may be NULL on all but one of them.
 * Nothing outside rows [row0, row0 + n) of a destination and [0, n) of x_out / xi_out is touched.
 * Checked before anything is launched (PM_EINVAL, outputs untouched): n >= 1, 1 <= ntargets <= 8,
 * member0 >= 0; per entry len >= 1, row0 >= 0, n * len < 2^31, dst / base / sigma / x_in not NULL,
 * no entry's x_out equal to any entry's x_in, a and b finite and in [0, 1], pattern_per_member 0
 * or 1, 0 <= stream < PM_NOISE_STREAMS.                                                         */
#define PM_NOISE_MAX_TARGETS 8
#define PM_NOISE_STREAMS 6
typedef struct pm_noise_target {
  double *dst; int64_t row0;             /* rows [row0, row0 + n) of [.][len] are written         */
  const double *base;                    /* device [n][len]                                       */
  const double *pattern;                 /* device [len] or [n][len]; NULL: 1                     */
  const double *sigma;                   /* device [n]                                            */
  const double *x_in;                    /* device [n]                                            */
  double *x_out;                         /* device [n], not x_in; may be NULL                     */
  double *xi_out;                        /* device [n]: the deviates used; may be NULL            */
  double a, b;
  int32_t len, pattern_per_member, stream, reserved;
} pm_noise_target;
struct pm_noise {
  int32_t n, ntargets;
  uint32_t j, reserved;
  uint64_t seed;
  int64_t member0;
  pm_noise_target target[PM_NOISE_MAX_TARGETS];
};
/* the struct is named by its tag only, as pm_steady_check's is */
int pm_forcing_noise(const struct pm_noise *d, pm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Statistics of a recorded series (pymoc_amd.SeriesStats), reduced on the device: ONE launch per
 * entry.  (no counterpart: what a user computes in NumPy from the downloaded series.)  Both entries
 * read a series of doubles
 *   v[k][s][m],  k < nrec records, s < nspec indices, m < n members (members contiguous: an
 *   IndexRecorder's device layout)
 * over the record window [k0, k1).  A value is FINITE iff isfinite; non-finite values mark members
 * that blew up: they are excluded and counted, never propagated.  Every sum below has one order,
 * which is part of the ABI: it does not depend on the kernel variant, the block size or the launch
 * geometry, and with every product and sum rounded on its own (-ffp-contract=off) each double is
 * reproduced bit for bit by a NumPy restatement.
 *
 * pm_series_group_stats -- across the members of a group, per (record k in the window, index s,
 * group g):
 *   count[k][s][g]            (int32)
 *   stat[k][s][g][5 + nq]     mean, var, min, max, sum, q_0 .. q_{nq-1}
 * (both [nrec][nspec][ngroups]; records outside the window are not touched).  order[n] is a
 * permutation of the members sorted by group, ascending member index inside a group; group g is
 * order[start[g] .. start[g+1] - 1].  For the group's values x_0 .. x_{G-1} in that order:
 *   count   the number of finite x_j;  x'_j = x_j if x_j is finite, else +0.0
 *   sum     p[l], l < 64, is the sequential sum in ascending j of the x'_j with j = l (mod 64),
 *           starting from +0.0; then for stride = 32, 16, 8, 4, 2, 1: p[l] += p[l + stride] for
 *           l < stride; sum = p[0]
 *   mean    sum / count
 *   var     Q / (count - 1), Q the same tree over d_j * d_j with d_j = x_j - mean for finite x_j
 *           and 0 otherwise; NaN for count < 2
 *   min, max  the first and the last of the finite values sorted ascending, -0.0 before +0.0: the
 *           very bits
 *   q_i     NumPy's method="linear" on the sorted finite values: m = count, vi = q * (m - 1),
 *           lo = floor(vi), hi = min(lo + 1, m - 1), g = vi - lo, a = sorted[lo], b = sorted[hi];
 *           g >= 0.5 ? b - (b - a) * (1 - g) : a + (b - a) * g
 *   count = 0 stores NaN in every double of stat.  A group of size 0 is allowed (count 0).
 * Groups of at most 64 members are reduced by one wavefront in registers, larger ones (at most
 * PM_STATS_GROUP_MAX, sorted in 64 KiB of LDS) by a workgroup; sizes may differ within a launch,
 * and every value of the window is read once.
 *
 * pm_series_member_stats -- along the records, per (index s, member m):
 *   count[s][m], first[s][m], ncross[s][m]   (int32)
 *   stat[s][m][6 + nlag]                     mean, var, min, max, sum, frac, c_{L_0} ..
 * The records of the window are cut into chunks of PM_STATS_CHUNK consecutive records counted from
 * k0.  A chunk's partial is the sequential sum in ascending k of its terms, starting from +0.0; a
 * total is the sequential sum of the chunk partials in ascending order, starting from +0.0.
 *   count   the number of finite records;  sum: the total of x'_k (x_k if finite, else +0.0)
 *   mean    sum / count;  var = Q / (count - 1), Q the total of d_k * d_k, d_k = x_k - mean for
 *           finite x_k and 0 otherwise; NaN for count < 2
 *   min, max  over the finite records; of -0.0 and +0.0, min takes -0.0 and max +0.0
 *   c_L     the total, over the k with x_k and x_{k+L} both finite and both inside the window, of
 *           (x_k - mean) * (x_{k+L} - mean) (other k contribute +0.0; a pair belongs to the chunk
 *           of k), divided by the number of such pairs; NaN with no such pair
 *   thr[s] = t (NaN: none), dir[s] = d: x_k is a HIT iff it is finite and x_k < t (d = -1) or
 *           x_k > t (d = +1).  frac = hits / count; first = the smallest hit k (an absolute record
 *           number), -1 if none; ncross = the number of k with x_k and x_{k+1} both finite, both
 *           inside the window, and exactly one of them a hit.  Without a threshold: NaN, -1, 0
 *   count = 0 stores NaN in mean, var, min, max (and frac), and sum = +0.0.
 *
 * Checked before anything is launched (PM_EINVAL, outputs untouched): no NULL pointer where one is
 * read or written (q / lag may be NULL with nq / nlag = 0); n, nspec, nrec >= 1 (nspec <= 65535,
 * (k1 - k0) * nspec < 2^30); 0 <= k0 < k1 <= nrec; ngroups >= 1; 0 <= nq <= PM_STATS_Q_MAX,
 * every q in [0, 1] and not NaN; 0 <= nlag <= PM_STATS_LAG_MAX, every L in [1, k1 - k0); dir -1 or
 * +1; start[0] = 0, start monotone, start[ngroups] = n, no group larger than PM_STATS_GROUP_MAX.
 * The checks read the HOST mirrors (start, q, lag, thr, dir); the kernels read the device copies
 * of the same values.  That order is a permutation of 0 .. n-1 is the caller's to ensure.     */
#define PM_STATS_Q_MAX 8
#define PM_STATS_LAG_MAX 4
#define PM_STATS_GROUP_MAX 8192
#define PM_STATS_CHUNK 256
struct pm_series_group_stats {
  int32_t n, nspec, nrec, k0, k1, ngroups, nq, reserved;
  const double *v;                       /* device [nrec][nspec][n]                               */
  const int32_t *order;                  /* device [n]                                            */
  const int32_t *start;                  /* HOST [ngroups + 1]                                    */
  const int32_t *start_dev;              /* DEVICE, the same values                               */
  const double *q;                       /* HOST [nq]                                             */
  const double *q_dev;                   /* DEVICE, the same values                               */
};
/* the struct is named by its tag only, as pm_steady_check's is */
int pm_series_group_stats(const struct pm_series_group_stats *d, int32_t *count, double *stat,
                          pm_stream_t stream);
struct pm_series_member_stats {
  int32_t n, nspec, nrec, k0, k1, nlag, reserved1, reserved2;
  const double *v;                       /* device [nrec][nspec][n]                               */
  const int32_t *lag;                    /* HOST [nlag]                                           */
  const int32_t *lag_dev;                /* DEVICE, the same values                               */
  const double *thr;                     /* HOST [nspec]; NaN: no threshold                       */
  const double *thr_dev;                 /* DEVICE, the same values                               */
  const int32_t *dir;                    /* HOST [nspec]: -1 below, +1 above                      */
  const int32_t *dir_dev;                /* DEVICE, the same values                               */
};
int pm_series_member_stats(const struct pm_series_member_stats *d, int32_t *count, int32_t *first,
                           int32_t *ncross, double *stat, pm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Welch power and cross spectra of a recorded series (pymoc_amd.SeriesSpectra), on the device: ONE
 * launch.  (no counterpart: what a user computes with scipy.signal.welch / scipy.signal.csd from
 * the downloaded series.)  The series is v[k][s][m] as above, the record window [k0, k1),
 * K = k1 - k0, L = nperseg.
 *   L is a power of two, PM_SPEC_NPERSEG_MIN = 8 <= L <= PM_SPEC_NPERSEG_MAX = 1024;  K >= L
 *   the step between segments is S = step = L - noverlap, 1 <= S <= L
 *   segment i, i < nseg = (K - L) / S + 1, holds the records k0 + i*S + j, j < L
 *   no padding and no partial segment: the records behind the last whole segment are not read
 * For one series x a segment is USED iff all L of its values are finite (isfinite); the other
 * segments are excluded and counted, never propagated.  For a used segment:
 *   1. detrend and window.  PM_SPEC_DETREND_CONSTANT: mu = the sequential sum of x_j in ascending
 *      j, starting from +0.0, divided by L; y_j = (x_j - mu) * w_j.  PM_SPEC_DETREND_NONE:
 *      y_j = x_j * w_j.  w[L] is the window the caller passes.
 *   2. transform.  Z = DFT(y + 0i) with the rounding of the iterative radix-2 decimation-in-time
 *      transform: a[j] = y[bitrev(j)]; for the stages h = 1, 2, 4 .. L/2, every block base b (a
 *      multiple of 2h) and every q < h, with W = tw[q * (L / (2h))], u = a[b+q], v = a[b+q+h]:
 *        tr = W.re*v.re - W.im*v.im      ti = W.re*v.im + W.im*v.re
 *        a[b+q] = u + (tr, ti)           a[b+q+h] = u - (tr, ti)
 *      every product and sum rounded on its own (-ffp-contract=off).  tw[j] = (cos(2 pi j / L),
 *      -sin(2 pi j / L)), j < L/2, is a table the caller passes (twiddle[j][2]: re, im); the
 *      kernel calls no sin or cos.  (An implementation may fuse stages or skip work on known
 *      zeros as long as it reproduces these bits.)
 *   3. periodogram.  p_i[f] = Z.re*Z.re + Z.im*Z.im, f = 0 .. L/2 (nf = L/2 + 1).  For a pair
 *      (a, b): c_i[f] = conj(Z_a) * Z_b (SciPy's convention),
 *        re = Za.re*Zb.re + Za.im*Zb.im      im = Za.re*Zb.im - Za.im*Zb.re
 *      and a pair's segment is used iff it is used for both series.
 * Results, members contiguous in each:
 *   nused[s][m], nused_pair[p][m]   (int32) the number of used segments
 *   psd[f][s][m]                    ((acc[f] / nused) * scale) * c, acc[f] the sequential sum of
 *                                   p_i[f] over the used segments in ascending i, starting from
 *                                   +0.0; c = 1 at f = 0 and f = L/2, else 2 (one-sided);
 *                                   scale = 1 / (fs * sum w^2) is the caller's, one double
 *   csd[f][2p + {0, 1}][m]          the same of the real and of the imaginary part of c_i[f]
 * nused = 0 stores NaN.  psd is itself a series [nf][nspec][n] that pm_series_group_stats reads
 * as it stands.  The result of a series or of a pair depends on that member's values alone: not
 * on the member's position in the batch, its neighbours, n or the launch geometry.
 *
 * Checked before anything is launched (PM_EINVAL, outputs untouched): no NULL pointer where one is
 * read or written (pair, nused_pair and csd may be NULL iff npairs = 0); n, nspec, nrec >= 1;
 * 0 <= k0 < k1 <= nrec; L a power of two in [8, 1024]; K >= L; 1 <= step <= L; a known detrend;
 * 0 <= npairs <= PM_SPEC_PAIRS_MAX, every pair index in [0, nspec); every window value and scale
 * finite; nf * nspec < 2^30; nspec + npairs <= 65535.  The checks read the HOST mirrors (window,
 * pair); the kernel reads the device copies of the same values.                              */
#define PM_SPEC_NPERSEG_MIN 8
#define PM_SPEC_NPERSEG_MAX 1024
#define PM_SPEC_PAIRS_MAX 8
#define PM_SPEC_DETREND_NONE 0
#define PM_SPEC_DETREND_CONSTANT 1
struct pm_series_spectra {
  int32_t n, nspec, nrec, k0, k1, nperseg, step, detrend, npairs, reserved;
  const double *v;                       /* device [nrec][nspec][n]                               */
  const double *window;                  /* HOST [nperseg]                                        */
  const double *window_dev;              /* DEVICE, the same values                               */
  const double *twiddle;                 /* device [nperseg / 2][2]                               */
  const int32_t *pair;                   /* HOST [npairs][2]                                      */
  const int32_t *pair_dev;               /* DEVICE, the same values                               */
  double scale;
};
int pm_series_spectra(const struct pm_series_spectra *d, int32_t *nused, double *psd,
                      int32_t *nused_pair, double *csd, pm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Sliding-window early-warning indicators of a recorded series and the Kendall trend of a series
 * against its record number (pymoc_amd.SeriesWindows), on the device: ONE launch per entry.  (no
 * counterpart: what a user computes with a rolling apply over the downloaded series.)  The series
 * is v[k][s][m] as above, the record window [k0, k1), K = k1 - k0.
 *
 * pm_series_windows -- W = window, S = step, Lg = lag:
 *   PM_WIN_MIN = 4 <= W <= PM_WIN_MAX = 4096 (any W, not only powers of two);  K >= W
 *   1 <= S <= W;  1 <= Lg <= W - 2
 *   window i, i < nwin = (K - W) / S + 1, holds the records k0 + i*S + j, j < W
 *   no partial window: the records behind the last whole window are not read
 * For one series x a window is USED iff all W of its values are finite (isfinite); the other
 * windows are excluded and counted, never propagated.  For a used window, every product and sum
 * rounded on its own (-ffp-contract=off), every sum sequential in ascending j from +0.0:
 *   t_j   = (double)j - 0.5 * (W - 1)                                  (exact)
 *   stt   = sum t_j^2 = W (W^2 - 1) / 12, one double the caller passes; the entry checks it against
 *           its own evaluation
 *   pass 1  s = sum x_j;  st = sum t_j * x_j
 *   mean  = s / W
 *   slope = st / stt for PM_WIN_DETREND_LINEAR; +0.0 for _CONSTANT and _NONE
 *   r_j   = (x_j - mean) - slope * t_j   LINEAR
 *           x_j - mean                   CONSTANT
 *           x_j                          NONE
 *   pass 2  q = sum_{j < W} r_j * r_j;  c = sum_{j < W - Lg} r_j * r_{j + Lg}
 *   var   = q / (W - 1)
 *   ac    = c / q: the biased autocorrelation estimate (R's acf, statsmodels), not the Pearson
 *           correlation of the shifted pair; NaN when q == 0
 * Results, members contiguous in each:
 *   out[4][nwin][nspec][n]   mean, slope, var, ac; an unused window stores NaN in all four.  Each
 *                            out[i] is itself a series [nwin][nspec][n] that
 *                            pm_series_group_stats and pm_series_kendall read as it stands
 *   nused[nspec][n]          (int32) the number of used windows
 * The result of a series depends on that member's values alone: not on the member's position in
 * the batch, its neighbours, n or the launch geometry -- windows are independent, so a block may
 * take any range of them.  pm_series_windows_geometry reports the tile of a (W, S): the adjacent
 * members and the consecutive windows one block takes.
 *
 * pm_series_kendall -- per (index s, member m), over the pairs a < b of records of the window with
 * x_a and x_b both finite:
 *   conc[s][m]   the number of pairs with x_b > x_a
 *   disc[s][m]   ... with x_b < x_a
 *   tie[s][m]    ... with x_b == x_a
 *   nfin[s][m]   the number of finite records
 * (all int32; K <= PM_KENDALL_MAX = 4096, so K (K - 1) / 2 < 2^23).  Exact integers: no order and
 * nothing to round.  tau-b against time, which has no ties, is the caller's to form:
 * (conc - disc) / sqrt(n0 * (n0 - tie)), n0 = conc + disc + tie.
 *
 * Checked before anything is launched (PM_EINVAL, outputs untouched): no NULL pointer where one is
 * read or written; n, nspec, nrec >= 1; 0 <= k0 < k1 <= nrec; W, S, Lg in the ranges above;
 * K >= W; a known detrend; stt equal to the entry's own value; nwin * nspec < 2^30;
 * nspec <= 65535; (member tiles) * (window chunks) < 2^31; K <= PM_KENDALL_MAX for the trend.  */
#define PM_WIN_MIN 4
#define PM_WIN_MAX 4096
#define PM_WIN_DETREND_NONE 0
#define PM_WIN_DETREND_CONSTANT 1
#define PM_WIN_DETREND_LINEAR 2
#define PM_KENDALL_MAX 4096
struct pm_series_windows {
  int32_t n, nspec, nrec, k0, k1, window, step, lag, detrend, reserved;
  const double *v;                       /* device [nrec][nspec][n]                               */
  double stt;                            /* W (W^2 - 1) / 12                                      */
};
int pm_series_windows(const struct pm_series_windows *d, double *out, int32_t *nused,
                      pm_stream_t stream);
int pm_series_windows_geometry(int32_t window, int32_t step, int32_t *members, int32_t *windows);
struct pm_series_kendall {
  int32_t n, nspec, nrec, k0, k1, reserved1, reserved2, reserved3;
  const double *v;                       /* device [nrec][nspec][n]                               */
};
int pm_series_kendall(const struct pm_series_kendall *d, int32_t *conc, int32_t *disc,
                      int32_t *tie, int32_t *nfin, pm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * pm_series_dfa -- the detrended-fluctuation-analysis exponent (Livina & Lenton 2007; the third
 * indicator of Lenton et al. 2012) of every sliding window, on the device: ONE launch.  (no
 * counterpart: a rolling Python loop over the downloaded series.)  The series, the record window,
 * W = window, S = step, detrend and stt are pm_series_windows': the same windows, the same rule
 * (a window is USED iff all W of its values are finite).  Besides them the entry takes nq scales
 *   s_0 < s_1 < .. < s_{nq-1},   2 <= nq <= PM_DFA_SCALES_MAX = 16,
 *   PM_DFA_SCALE_MIN = 4 <= s_0,  4 * s_{nq-1} <= W      (at least four boxes per scale: W >= 20)
 * and two HOST-made tables of nq doubles, suu and weight (below).
 * For a used window, every product and sum rounded on its own (-ffp-contract=off), every sum
 * sequential in ascending order from +0.0:
 *   pass 1   mean and slope exactly as pm_series_windows forms them (the same order: the same bits)
 *   d_j      = r_j of pm_series_windows under LINEAR and CONSTANT; under NONE d_j = x_j - mean
 *              (the profile of DFA is that of the mean-removed series by definition)
 *   per scale s = s_q:
 *     nb     = W / s boxes (integer division) from the window's start, box b holding the records
 *              j = b s + i, i < s; the W - nb s trailing records belong to no box
 *     u_i    = (double)i - 0.5 * (s - 1)                                     (exact)
 *     suu_q  = sum u_i^2 = s (s^2 - 1) / 12, the table suu[q]; the entry checks it against its own
 *              evaluation bit for bit, as it does stt
 *     the profile y runs over the window from +0.0, y <- y + d_j, and f_q over all boxes of the
 *     scale from +0.0; per box, sy and su from +0.0:
 *       pass A   over the box's s records:  y <- y + d_j;  sy <- sy + y;  su <- su + u_i * y
 *                a = sy / (double)s;  c = su / suu_q
 *       pass B   y restarts from its value at the box's start; over the same records:
 *                y <- y + d_j;  e = (y - a) - c * u_i;  f_q <- f_q + e * e
 *     F2_q   = f_q / (double)(nb * s)
 *   alpha    = sum_q weight[q] * log(F2_q), sequential in q from +0.0, log the natural logarithm;
 *              weight[q] = 0.5 (L_q - Lbar) / sum_q (L_q - Lbar)^2 with L_q = ln s_q and Lbar their
 *              mean: the least-squares slope of ln F against ln s.  The entry checks that the
 *              weights are finite and sum to zero within rounding (|sum| <= 2^-40 sum |w|).
 *              alpha is NaN unless every F2_q is finite and > 0 (a constant window, an overflow).
 * F2_q is defined by IEEE operations alone and is reproduced bit for bit; alpha goes through the
 * device library's log and is stated to a bound (tests/dfa_cases.py).
 * Results, members contiguous in each:
 *   alpha[nwin][nspec][n]
 *   f2[nq][nwin][nspec][n]    stored iff f2 != NULL
 * an unused window stores NaN in every plane; each plane is a series that pm_series_kendall and
 * pm_series_group_stats read as it stands.  (The number of used windows is pm_series_windows'.)
 * A result depends on that member's values alone, as for pm_series_windows.
 *
 * Checked before anything is launched (PM_EINVAL, outputs untouched): what pm_series_windows
 * checks of n, nspec, nrec, [k0, k1), W, S, K >= W, detrend, stt, nwin * nspec, nspec and the
 * grid; nq and the scales in the ranges above and strictly ascending; both tables; v and alpha
 * not NULL.                                                                                    */
#define PM_DFA_SCALES_MAX 16
#define PM_DFA_SCALE_MIN 4
struct pm_series_dfa {
  int32_t n, nspec, nrec, k0, k1, window, step, detrend, nq, reserved;
  const double *v;                       /* device [nrec][nspec][n]                               */
  double stt;                            /* W (W^2 - 1) / 12                                      */
  int32_t scale[PM_DFA_SCALES_MAX];      /* s_q, q < nq (the rest is not read)                    */
  double suu[PM_DFA_SCALES_MAX];         /* s_q (s_q^2 - 1) / 12                                  */
  double weight[PM_DFA_SCALES_MAX];      /* of log(F2_q) in alpha                                 */
};
int pm_series_dfa(const struct pm_series_dfa *d, double *alpha, double *f2, pm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * pm_series_restoring -- the restoring rate lambda of every sliding window under AR(1)-correlated
 * regression errors (Boers 2021: the increments of the detrended index regressed on the index,
 * by iterated generalised least squares), on the device: ONE launch.  (no counterpart: a rolling
 * statsmodels GLSAR fit over the downloaded series.)  The series, the record window, W = window,
 * S = step, detrend and stt are pm_series_windows': the same windows, the same rule (a window is
 * USED iff all W of its values are finite).  Besides them the entry takes iters.
 *   PM_RESTORE_WIN_MIN = 8 <= W <= PM_WIN_MAX;  1 <= iters <= PM_RESTORE_ITERS_MAX = 64
 * For a used window, every product, sum and quotient rounded on its own (-ffp-contract=off), every
 * sum sequential in ascending order from +0.0, every expression evaluated as it is parenthesised
 * (left to right where it is not):
 *   pass 1   mean and slope exactly as pm_series_windows forms them (the same order: the same bits)
 *   d_j      = r_j of pm_series_windows under LINEAR and CONSTANT; under NONE d_j = x_j - mean
 *              (lambda with an intercept does not depend on an offset, and the offset must not
 *              cost digits)
 *   N = W - 1;  x_t = d_t,  y_t = d_{t+1} - d_t  for t < N;  M = N - 1
 *   pass 2   over t = 1 .. N - 1 ascending, with (xc, yc) = (x_t, y_t), (xp, yp) = (x_{t-1},
 *            y_{t-1}), the fourteen sums
 *              Sxc = sum xc     Sxp = sum xp     Syc = sum yc     Syp = sum yp
 *              Sxcxc = sum xc * xc     Sxcxp = sum xc * xp     Sxpxp = sum xp * xp
 *              Sxcyc = sum xc * yc     Sxcyp = sum xc * yp     Sxpyc = sum xp * yc
 *              Sxpyp = sum xp * yp     Sycyc = sum yc * yc     Sycyp = sum yc * yp
 *              Sypyp = sum yp * yp
 *            x_0 and y_0 are kept aside.  (No expression below reads Sypyp: the squared residuals
 *            are summed over the current pairs plus the t = 0 term.  An implementation need not
 *            form it.)  Then, once:  Sxy2 = Sxcyp + Sxpyc;  Sy2 = Syc + Syp;  Sx2 = Sxc + Sxp
 *   rho_0 = +0.0.  For i = 0 .. iters - 1, a fixed count with no early exit, with r = rho_i and
 *   Mf = (double)M:
 *     r2  = r * r
 *     SX  = Sxc - r * Sxp                                  the sums over t = 1 .. N - 1 of the
 *     SY  = Syc - r * Syp                                  whitened X* = x_t - r x_{t-1} and
 *     SXX = (Sxcxc - (2.0 * r) * Sxcxp) + r2 * Sxpxp       Y* = y_t - r y_{t-1}; the first
 *     SXY = (Sxcyc - r * Sxy2) + r2 * Sxpyp                observation is dropped, as GLSAR's
 *     mx  = SX / Mf;  my = SY / Mf                         whitening drops it
 *     lambda_i = (SXY - SX * my) / (SXX - SX * mx)
 *   and, for i < iters - 1 only (the last lambda needs no further rho):
 *     a   = (my - lambda_i * mx) / (1.0 - r)               the intercept of the unwhitened model
 *     e0  = (y_0 - a) - lambda_i * x_0                     its residual at t = 0
 *     l2  = lambda_i * lambda_i;  al = a * lambda_i;  a2m = Mf * (a * a)
 *     q   = (((((Sycyc - (2.0 * a) * Syc) - (2.0 * lambda_i) * Sxcyc) + (2.0 * al) * Sxc)
 *            + l2 * Sxcxc) + a2m) + e0 * e0                = sum_{t < N} e_t^2
 *     c   = ((((Sycyp - a * Sy2) - lambda_i * Sxy2) + al * Sx2) + l2 * Sxcxp) + a2m
 *                                                          = sum_{t = 1}^{N-1} e_t e_{t-1}
 *     rho_{i+1} = c / q      with e_t = y_t - a - lambda_i x_t: the biased lag-1 estimate, as
 *                            pm_series_windows' ac, so |rho| <= 1 before rounding (statsmodels'
 *                            GLSAR demeans the residuals and uses the adjusted Yule-Walker
 *                            estimate; this is not that)
 *   lam = lambda_{iters-1};  rho = rho_{iters-1}, the rho the stored lambda was fitted with (+0.0
 *   for iters = 1: ordinary least squares over t >= 1).  Both are NaN unless both are finite.  A
 *   constant window, a window the line fits exactly (q = 0) and an overflow follow what IEEE
 *   gives: there is no special case.
 * lambda is per record interval: lambda = phi - 1 for an AR(1) state with coefficient phi, -dt /
 * tau for a relaxation time tau sampled every dt; it rises towards 0 as stability is lost.
 * Neither sqrt, log nor exp is called: lam and rho are defined by IEEE operations alone and are
 * reproduced bit for bit (tests/restoring_cases.py).
 * Results, members contiguous in each:
 *   lam[nwin][nspec][n]
 *   rho[nwin][nspec][n]    stored iff rho != NULL
 * an unused window stores NaN in both; each is a series that pm_series_kendall and
 * pm_series_group_stats read as it stands.  (The number of used windows is pm_series_windows'.)
 * A result depends on that member's values alone, as for pm_series_windows.
 *
 * Checked before anything is launched (PM_EINVAL, outputs untouched): what pm_series_windows
 * checks of n, nspec, nrec, [k0, k1), S, K >= W, detrend, stt, nwin * nspec, nspec and the grid;
 * W and iters in the ranges above; v and lam not NULL.                                          */
#define PM_RESTORE_WIN_MIN 8
#define PM_RESTORE_ITERS_MAX 64
struct pm_series_restoring {
  int32_t n, nspec, nrec, k0, k1, window, step, detrend, iters, reserved;
  const double *v;                       /* device [nrec][nspec][n]                               */
  double stt;                            /* W (W^2 - 1) / 12                                      */
};
int pm_series_restoring(const struct pm_series_restoring *d, double *lam, double *rho,
                        pm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Surrogate significance of the trends above (pymoc_amd.SeriesSurrogates,
 * SeriesWindows.significance), on the device: ONE launch per entry and chunk of surrogates.  (no
 * counterpart: what a user does with a random generator and a loop over the downloaded series.)
 *
 * pm_series_surrogates -- nb stationary AR(1) surrogates of every (index s, member m) series,
 * written as a device series of K records in the layout above:
 *   y[j][p][m],  j < K, p = i * nspec + s for surrogate b = b0 + i (i < nb, b0 the GLOBAL number of
 *   the chunk's first surrogate), m < n -- a series of nb * nspec indices that pm_series_windows,
 *   pm_series_kendall, pm_series_member_stats and pm_series_spectra read as it stands
 * from the two fit values var[s][m] and ac[s][m]: planes out[2] and out[3] of pm_series_windows
 * with ONE window spanning the record window (window = K, step = 1, lag = 1), hence
 * K <= PM_SURROGATE_MAX = PM_WIN_MAX.  Per (b, s, m), every product and sum rounded on its own
 * (-ffp-contract=off):
 *   phi  = ac[s][m];  sd = sqrt(var[s][m]);  g = sd * sqrt(fmax(0.0, 1.0 - phi * phi))
 *   xi_j = xi(seed, member0 + m, b, (s << 12) | j): the deviate of pm_forcing_noise above with the
 *          Philox counter words { id_lo, id_hi, b, (s << 12) | j } -- the surrogate number takes
 *          the slot `j` has there and (index, record) take the slot of `stream`; j < 4096 and
 *          s <= 65535, so the packing is one to one.  (A NoiseForcing bound with the same seed uses
 *          stream < PM_NOISE_STREAMS, that is s = 0 and j < 6 here: give the surrogates a seed of
 *          their own where that matters.)
 *   y_0  = sd * xi_0;   y_j = phi * y_{j-1} + g * xi_j
 * sqrt and fmax are IEEE; only xi carries the tolerance stated above, so y equals the recurrence
 * fed the deviates the device used (xi_out) bit for bit.  If phi or sd is not finite (a record
 * window with a non-finite value, a constant series, var = inf) all K values of that series are
 * NaN: stored, never skipped, so every entry above excludes and counts the series by its own rule.
 * xi_out (may be NULL) has y's shape and holds the deviates used, of the NaN series too.  A
 * surrogate depends on nothing but (seed, member0 + m, b, s, j) and its two fit values: not on n,
 * on the shard, on the chunk [b0, b0 + nb) or on the launch geometry.
 * Checked before the launch (PM_EINVAL, outputs untouched): no NULL pointer where one is read or
 * written (xi_out may be NULL); n, nspec, nb >= 1; 1 <= K <= PM_SURROGATE_MAX; b0 >= 0 and
 * b0 + nb <= 2^32; member0 >= 0; nb * nspec <= 65535 (the planes are the indices of the entries
 * that read y); K * nb * nspec < 2^31; nb * nspec * n < 2^31.
 *
 * pm_series_exceed -- per (index s, member m), how many of nb surrogate trends reach the observed
 * one.  From the counts of pm_series_kendall, observed [nspec][n] and surrogate [nb * nspec][n]
 * (plane i * nspec + s), with
 *   tau(c, d, t) = (double)(c - d) / sqrt((double)n0 * (double)(n0 - t)),  n0 = c + d + t
 * (operands exact: counts below 2^23, the product below 2^46; sqrt and the division correctly
 * rounded, so a NumPy restatement gives every tau bit for bit; NaN when n0 == t):
 *   if tau_obs is NaN nothing is added; otherwise for each of the nb surrogates whose tau is not
 *   NaN:  nvalid[s][m] += 1;  ge[s][m] += (tau_sur >= tau_obs);  le[s][m] += (tau_sur <= tau_obs)
 * ge, le and nvalid (int32 [nspec][n]) are ADDED to: the caller zeroes them once and calls the
 * entry once per chunk, on one stream; integer sums, so the chunking does not show.
 * Checked before the launch (PM_EINVAL, outputs untouched): no NULL pointer; n, nspec, nb >= 1;
 * nb * nspec <= 65535; nb * nspec * n < 2^31.                                                   */
#define PM_SURROGATE_MAX 4096
struct pm_series_surrogates {
  int32_t n, nspec, K, nb;
  int64_t b0;                            /* the GLOBAL number of the chunk's first surrogate      */
  int64_t member0;                       /* the GLOBAL number of member 0                         */
  uint64_t seed;
  const double *var;                     /* device [nspec][n]                                     */
  const double *ac;                      /* device [nspec][n]                                     */
};
int pm_series_surrogates(const struct pm_series_surrogates *d, double *y, double *xi_out,
                         pm_stream_t stream);
struct pm_series_exceed {
  int32_t n, nspec, nb, reserved;
  const int32_t *obs_conc, *obs_disc, *obs_tie;   /* device [nspec][n]                            */
  const int32_t *sur_conc, *sur_disc, *sur_tie;   /* device [nb * nspec][n]                       */
};
int pm_series_exceed(const struct pm_series_exceed *d, int32_t *ge, int32_t *le, int32_t *nvalid,
                     pm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Kernel detrending of a recorded series (pymoc_amd.SeriesSmooth, SeriesWindows(detrend =
 * "gaussian")), on the device: ONE launch.  (no counterpart: what a user computes with
 * scipy.ndimage.gaussian_filter1d or R's ksmooth over the downloaded series.)  The series is
 * v[k][s][m] as above, the record window [k0, k1), K = k1 - k0, 1 <= K <= PM_SMOOTH_MAX = 4096, and
 * x_j = v[k0 + j][s][m], j < K.
 * The caller passes a half-width H = half, 1 <= H <= PM_SMOOTH_HALF_MAX = 4095, and a weight table
 * w[0 .. H] with w[0] == 1.0, every w[d] finite and > 0 and w[d + 1] <= w[d] (for a Gaussian of
 * sigma records: w[d] = exp(-0.5 (d / sigma)^2)); the device evaluates no exp.  Per record j, with
 *   lo = max(0, j - H),  hi = min(K - 1, j + H)
 * every product and sum rounded on its own (-ffp-contract=off), both sums sequential in ascending
 * i from +0.0 over the i in [lo, hi] with isfinite(x_i) only:
 *   num     = sum w[|i - j|] * x_i
 *   den     = sum w[|i - j|]
 *   trend_j = num / den                       NaN when no record in reach is finite (0 / 0)
 *   resid_j = x_j - trend_j if isfinite(x_j), else NaN
 *   nbad[s][m] = the number of non-finite records of the record window
 * A non-finite record is left out and counted, never propagated: the trend at such a record is the
 * gap-filled value from its neighbours, its residual is NaN (pm_series_windows then excludes every
 * window that holds it, by its own rule).  The edges are renormalised by den (Nadaraya-Watson, as
 * R's ksmooth), not reflected: a record outside [k0, k1) is never read.
 * Results, members contiguous in each:
 *   trend[K][nspec][n], resid[K][nspec][n]   each a series of its own that every pm_series_* entry
 *                                            reads as it stands; either may be NULL and is then not
 *                                            stored
 *   nbad[nspec][n]                           (int32)
 * The result of a series depends on that member's values alone: not on the member's position in
 * the batch, its neighbours, n or the launch geometry -- records are independent, so a block may
 * take any range of them.  pm_series_smooth_geometry reports the tile of an H: the adjacent members
 * and the consecutive records one block takes.
 *
 * Checked before anything is launched (PM_EINVAL, outputs untouched): no NULL pointer where one is
 * read or written (trend or resid may be NULL, not both); n, nspec, nrec >= 1; 0 <= k0 < k1 <= nrec;
 * K <= PM_SMOOTH_MAX; H in [1, PM_SMOOTH_HALF_MAX]; the table conditions; nspec <= 65535; (member
 * tiles) * (record chunks) < 2^31.  The checks read the HOST table w; the kernel reads the device
 * copy of the same values.                                                                      */
#define PM_SMOOTH_MAX 4096
#define PM_SMOOTH_HALF_MAX 4095
struct pm_series_smooth {
  int32_t n, nspec, nrec, k0, k1, half, reserved1, reserved2;
  const double *v;                       /* device [nrec][nspec][n]                               */
  const double *w;                       /* HOST [half + 1]                                       */
  const double *w_dev;                   /* DEVICE, the same values                               */
};
int pm_series_smooth(const struct pm_series_smooth *d, double *trend, double *resid, int32_t *nbad,
                     pm_stream_t stream);
int pm_series_smooth_geometry(int32_t half, int32_t *members, int32_t *records);
/* The LDS bytes one block of a launch with this half-width over nrecords = K records asks for (all
 * dynamic: the kernel has no static LDS); at most the 160 KiB of a CU for every valid (H, K).   */
int pm_series_smooth_lds_bytes(int32_t half, int32_t nrecords, size_t *bytes);

/* ---------------------------------------------------------------------------------------------
 * Abrupt shifts of a recorded series and per-member analysis ends (pymoc_amd.SeriesShifts,
 * SeriesWindows.significance(until=)), on the device: ONE launch per entry.  (no counterpart: what
 * a user does with a rolling two-window statistic and per-member slices of the downloaded series.)
 * The series is v[k][s][m] as above, the record window [k0, k1), K = k1 - k0; records are numbered
 * from k0 in everything below.  Every product and sum is rounded on its own (-ffp-contract=off);
 * division and sqrt are IEEE.
 *
 * pm_series_shift_scan -- the largest shift between two adjacent windows of L = half records, from
 * quantities pm_series_windows has already formed (so no sum gets a second order):
 *   PM_WIN_MIN <= L <= PM_SHIFT_HALF_MAX = 2048;  2 L <= K
 *   mean, var   the planes out[0] and out[2] of pm_series_windows over the same record window with
 *               window = L, step = 1, PM_WIN_DETREND_CONSTANT, lag = 1: each [nwin][nspec][n],
 *               nwin = K - L + 1, window i covering the records [i, i + L)
 * Per (index s, member m) and candidate c = L .. K - L:
 *   jump   = mean[c] - mean[c - L]
 *   pooled = 0.5 * (var[c - L] + var[c])
 *   stat   = jump / sqrt(pooled)           pooled == 0: +-inf, NaN when jump == 0 too
 *   score  = -stat (dir[s] = -1: drops), fabs(stat) (dir[s] = 0), stat (dir[s] = +1: rises)
 * A candidate COUNTS iff mean[c - L] and mean[c] are not NaN and its score is not NaN (an infinite
 * score counts).  Results, members contiguous in each:
 *   at[s][m]      (int32) the counting candidate with the largest score, the smallest c among equal
 *                 scores (-0.0 == +0.0); -1 if none counts
 *   first[s][m]   (int32) the smallest counting c with score >= thr[s]; -1 if there is none or
 *                 thr[s] is NaN (no threshold)
 *   ncand[s][m]   (int32) the number of counting candidates
 *   val[4][nspec][n]   stat, jump, mean[c - L] and mean[c] at c = at; all four NaN when at = -1
 * The selection does not depend on the order the candidates are visited in, and a series' result
 * depends on that member's values alone: not on n, the shard or the launch geometry.
 * Checked before the launch (PM_EINVAL, outputs untouched): no NULL pointer; n, nspec, nrec >= 1;
 * 0 <= k0 < k1 <= nrec; L and K in the ranges above; nspec <= 65535; nwin * nspec < 2^30; every
 * dir in {-1, 0, +1}; no thr infinite.  The checks read the HOST mirrors (thr, dir); the kernel
 * reads the device copies of the same values.
 *
 * pm_series_censor -- a copy of a series with NaN from a per-member end on:
 *   y[j][p][m] = (j < end) ? x[j][p][m] : NaN,   j < K, p = i * nspec + s, i < nb, m < n
 *   w   = where[src[s]][m]
 *   end = w < 0 ? K : max(0, w - guard)
 * x and y are series of K records and nb * nspec indices (nb = 1: a record window of a recorded
 * series, passed by the address of its first record; nb > 1: the planes of pm_series_surrogates).
 * `where` (int32 [nspec][n], device) is `at` or `first` of the scan; src[s] names the index whose
 * shift governs index s (the identity: every index by its own).  Kept records are copied as bits
 * (a NaN keeps its payload); the NaN stored is the quiet NaN 0x7ff8000000000000.  y == x, in place,
 * is allowed; any other overlap is not.  end_out (int32 [nspec][n], may be NULL) receives end,
 * written once, not per plane.  Every pm_series_* entry excludes and counts the censored records
 * by its own rule; for pm_series_smooth that is an edge renormalised at `end`.
 * Checked before the launch (PM_EINVAL, outputs untouched): no NULL pointer where one is read or
 * written (end_out may be NULL); n, nspec, nb, K >= 1; guard >= 0; every src in [0, nspec);
 * nb * nspec <= 65535; K * nb * nspec < 2^31; nb * nspec * n < 2^31.  The check reads the HOST
 * mirror of src; the kernel reads the device copy.
 *
 * pm_series_fit_ranged -- the null-model fit of every member up to its own end.  Per (index s,
 * member m) with e = end[s][m]: var[s][m] and ac[s][m] are exactly what pm_series_windows defines
 * for ONE window over the records [k0, k0 + e) -- W = e, lag 1, the same two passes in the same
 * order, under detrend PM_WIN_DETREND_NONE, _CONSTANT or _LINEAR -- so they equal planes out[2] and
 * out[3] of that launch bit for bit.  stt of every W is read from the table stt_tab[0 .. K],
 * stt_tab[W] = W (W^2 - 1) / 12 (entries below PM_WIN_MIN are not read), which the entry checks
 * against its own evaluation.  e < PM_WIN_MIN, e > K, or a non-finite record inside the range
 * stores NaN in both values.  K <= PM_WIN_MAX.  var and ac are device [nspec][n], the shape
 * pm_series_surrogates reads.  A series' result depends on that member's values and end alone.
 * Checked before the launch (PM_EINVAL, outputs untouched): no NULL pointer; n, nspec, nrec >= 1;
 * 0 <= k0 < k1 <= nrec; K <= PM_WIN_MAX; a known detrend; nspec * n < 2^31; the table.  The check
 * reads the HOST table; the kernel reads the device copy of the same values.                   */
#define PM_SHIFT_HALF_MAX 2048
struct pm_series_shift_scan {
  int32_t n, nspec, nrec, k0, k1, half, reserved1, reserved2;
  const double *mean;                    /* device [k1 - k0 - half + 1][nspec][n]                 */
  const double *var;                     /* device, the same shape                                */
  const double *thr;                     /* HOST [nspec]; NaN: no threshold                       */
  const double *thr_dev;                 /* DEVICE, the same values                               */
  const int32_t *dir;                    /* HOST [nspec]: -1 drops, 0 either, +1 rises            */
  const int32_t *dir_dev;                /* DEVICE, the same values                               */
};
int pm_series_shift_scan(const struct pm_series_shift_scan *d, int32_t *at, int32_t *first,
                         int32_t *ncand, double *val, pm_stream_t stream);
struct pm_series_censor {
  int32_t n, nspec, K, nb, guard, reserved;
  const double *x;                       /* device [K][nb * nspec][n]                             */
  const int32_t *where;                  /* device [nspec][n]                                     */
  const int32_t *src;                    /* HOST [nspec]                                          */
  const int32_t *src_dev;                /* DEVICE, the same values                               */
};
int pm_series_censor(const struct pm_series_censor *d, double *y, int32_t *end_out,
                     pm_stream_t stream);
struct pm_series_fit_ranged {
  int32_t n, nspec, nrec, k0, k1, detrend, reserved1, reserved2;
  const double *v;                       /* device [nrec][nspec][n]                               */
  const int32_t *end;                    /* device [nspec][n]                                     */
  const double *stt_tab;                 /* HOST [k1 - k0 + 1]                                    */
  const double *stt_tab_dev;             /* DEVICE, the same values                               */
};
int pm_series_fit_ranged(const struct pm_series_fit_ranged *d, double *var, double *ac,
                         pm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Fourier phase-randomised surrogates of a recorded series (pymoc_amd.SeriesSurrogates(method =
 * "fourier"), SeriesWindows.significance(method = "fourier")), on the device: ONE launch per entry
 * and chunk of surrogates.  (no counterpart: what a user does with numpy.fft.rfft / irfft and a
 * loop over the downloaded series.)  A surrogate keeps the whole periodogram of the detrended
 * record window and randomises only the phases: the null model where the series is not AR(1).
 * Every product and sum is rounded on its own (-ffp-contract=off), and the device calls no sin,
 * cos, exp or sqrt: every trigonometric value comes from a table the caller passes, so a NumPy
 * restatement that reads the same arrays gives every double bit for bit.
 *
 * K = the records of the window, PM_WIN_MIN = 4 <= K <= PM_SURROGATE_MAX = 4096 (any K);
 * M = the smallest power of two with M >= 2K - 1 and M >= 8, so 8 <= M <= 8192.
 * Tables (each [..][2]: re, im), made once per K on the host:
 *   tw[M/2]     (cos(2 pi j / M), -sin(2 pi j / M)): pm_series_spectra's table at L = M
 *   chirp[K]    (cos(pi q / K), -sin(pi q / K)), q = j^2 mod 2K taken in integers
 *   filt[M]     the transform FFT_M below, in float64 with the same table tw, of b:
 *               b_j = conj(chirp_j) for j < K, b_{M-j} = b_j for 1 <= j < K, +0 elsewhere
 *   ph_hi[256]  e^{2 pi i a / 256};   ph_lo[256]  e^{2 pi i c / 65536}
 * The complex product x * c is  re = x.re*c.re - x.im*c.im,  im = x.re*c.im + x.im*c.re.
 * FFT_M(a) is the iterative radix-2 decimation-in-time transform exactly as stated for
 * pm_series_spectra above, of a complex a: a'[j] = a[bitrev(j)], then the stages h = 1 .. M/2 with
 * W = tw[q * (M / (2h))].
 *
 * BLU(x, sigma), the DFT of length K of a complex x with sign sigma (-1 forward, +1 inverse), by
 * Bluestein's chirp-z.  c^ = chirp for sigma = -1 and its conjugate for +1; B^ = filt, or its
 * conjugate, likewise (both conjugations exact; b is even, so its transform is even):
 *   a_j = x_j * c^_j for j < K, +0 for K <= j < M
 *   A   = FFT_M(a);   C_k = A_k * B^_k
 *   c   = conj(FFT_M(conj(C))) * (1 / M)           (a power of two)
 *   X_k = c_k * c^_k for k < K
 * (An implementation may fuse stages, skip work on known zeros or reorder independent operations
 * as long as it reproduces these bits.)
 *
 * pm_series_fourier_coef -- per (index s, member m) over the record window [k0, k1) of the series
 * v[k][s][m]: if any of the K records is not finite (isfinite) every coefficient of that series
 * is NaN.  Otherwise r_j is exactly the r_j pm_series_windows defines for ONE window of W = K
 * records under `detrend` (PM_WIN_DETREND_NONE, _CONSTANT or _LINEAR: the same sequential pass-1
 * sums, mean and slope; stt = K (K^2 - 1) / 12 is checked against the entry's own value), and
 *   R = BLU(r + 0i, -1);   coef[0][f][s][m] = R_f.re,  coef[1][f][s][m] = R_f.im,  f < nf = K/2 + 1
 * Each of the two planes is itself a series [nf][nspec][n] in the layout above.
 *
 * pm_series_surrogates_fourier -- per (surrogate b = b0 + i, s, m), written as y[j][i*nspec+s][m],
 * the layout of pm_series_surrogates:
 *   Z_0 = (R_0.re, +0);  for even K  Z_{K/2} = (R_{K/2}.re, +0);  for 1 <= f <= (K - 1) / 2:
 *     q = the top 16 bits of output word 0 of Philox4x32-10 keyed by the seed with the counter
 *         words { id_lo, id_hi, b, (s << 12) | f }, id = member0 + m  (f <= 2047: the packing is
 *         one to one)
 *     E = ph_hi[q >> 8] * ph_lo[q & 255];   Z_f = R_f * E;   Z_{K-f} = conj(Z_f)
 *   y_j = BLU(Z, +1)_j.re / (double)K
 * The phase is rotated, not replaced: |Z_f| = |R_f| up to rounding, without a sqrt; it is one of
 * 65536 values.  The counter is the one of pm_series_surrogates' deviate xi_f of the same
 * (seed, member, b, s): under the same seed the phase of frequency f and the AR(1) deviate of
 * record f come from the same Philox output (the phase from word 0's top 16 bits, the deviate
 * from all four words); give the two kinds of surrogate seeds of their own where that matters,
 * and a NoiseForcing too, as stated there.  A series with NaN coefficients has K NaN records:
 * stored, never skipped.  A surrogate depends on nothing but (seed, member0 + m, b, s) and that
 * series' coefficients: not on n, the shard, the chunk [b0, b0 + nb) or the launch geometry.
 * scratch (may be NULL) is a device array of y's size that must not overlap y: with one the entry
 * stores every series contiguously there and transposes it into y in a second launch -- the same
 * values, another store order, faster where a block holds a single series (M >= 2048); what scratch
 * holds afterwards is unspecified.
 *
 * Checked before the launch (PM_EINVAL, outputs untouched): no NULL pointer (but scratch); n, nspec >= 1 and
 * nrec >= 1, 0 <= k0 < k1 <= nrec (coef) or nb >= 1 (surrogates); PM_WIN_MIN <= K <=
 * PM_SURROGATE_MAX; M equal to the entry's own value for K; a known detrend and stt equal to the
 * entry's own value (coef); b0 >= 0, b0 + nb <= 2^32 and member0 >= 0; nspec <= 65535 and
 * nspec * n < 2^31 (coef); nb * nspec <= 65535, K * nb * nspec < 2^31 and nb * nspec * n < 2^31
 * (surrogates); every entry of the HOST mirrors of the tables finite.  The checks read the host
 * tables; the kernels read the device copies of the same values.                                */
struct pm_series_fourier_coef {
  int32_t n, nspec, nrec, k0, k1, detrend, M, reserved;
  const double *v;                       /* device [nrec][nspec][n]                               */
  double stt;                            /* K (K^2 - 1) / 12                                      */
  const double *tw, *chirp, *filt;       /* HOST [M/2][2], [K][2], [M][2]                         */
  const double *tw_dev, *chirp_dev, *filt_dev;   /* DEVICE, the same values                       */
};
int pm_series_fourier_coef(const struct pm_series_fourier_coef *d, double *coef,
                           pm_stream_t stream);
struct pm_series_surrogates_fourier {
  int32_t n, nspec, K, nb;
  int64_t b0;                            /* the GLOBAL number of the chunk's first surrogate      */
  int64_t member0;                       /* the GLOBAL number of member 0                         */
  uint64_t seed;
  int32_t M, reserved;
  const double *coef;                    /* device [2][K/2 + 1][nspec][n]                         */
  const double *tw, *chirp, *filt, *ph_hi, *ph_lo;   /* HOST [M/2][2], [K][2], [M][2], [256][2] x2 */
  const double *tw_dev, *chirp_dev, *filt_dev, *ph_hi_dev, *ph_lo_dev;   /* DEVICE, the same      */
  double *scratch;                       /* device [nb * nspec * n][K], or NULL                   */
};
int pm_series_surrogates_fourier(const struct pm_series_surrogates_fourier *d, double *y,
                                 pm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The leading EOF of several indices of a recorded series and its principal component
 * (pymoc_amd.SeriesEOF; Held & Kleinen 2004, "degenerate fingerprinting"), on the device: THREE
 * entries, one launch each.  (no counterpart: the download of the series and one
 * np.linalg.eigh per member.)  The series is v[k][s][m] as above, the record window [k0, k1),
 * K = k1 - k0 >= 2.  sel[q] holds q DISTINCT indices in [0, nspec), in any order,
 * 1 <= q <= PM_EOF_Q_MAX = 32; x_kj = v[k0 + k][sel[j]][m].  w[q][n] holds per-(index, member)
 * weights on the device; NULL: every weight is 1.0 (a product with 1.0 is exact: the same bits).
 * A UNIT is what shares one EOF: every member on its own (order, start and unit NULL, nu = n), or
 * a group of members, unit u = order[start[u] .. start[u+1] - 1], (order, start) as
 * pm_series_group_stats takes them, unit[m] the unit of member m.
 * Throughout: every product, sum and quotient is rounded on its own (-ffp-contract=off); every
 * sum is sequential in ascending order from +0.0; an argmax or a max is the FIRST on ties:
 *   first argmax of z_0 .. z_{q-1}:   p = 0; for i = 1 .. q - 1: if z_i > z_p then p = i
 *   first max of z_0 .. z_{q-1}:      the value z_p of that p
 * (a NaN never compares greater: a NaN z_0 stays, a later NaN is passed over).
 * Neither sqrt, log nor exp is called: every result is defined by IEEE operations alone and is
 * reproduced bit for bit by the NumPy restatement (tests/eof_cases.py).
 *
 * 1. pm_series_scatter -- per member m:
 *   record k is USED iff all q values x_kj are finite (isfinite)
 *   nused[m]   (int32) the number of used records
 *   mean_j   = (sum over the used k of x_kj) / (double)nused
 *   a_kj     = (x_kj - mean_j) * w_jm
 *   S_ij     = sum over the used k of a_ki * a_kj,  0 <= j <= i < q
 *   stores nused[n], mean[q][n], scat[q (q + 1) / 2][n] with S_ij at entry i (i + 1) / 2 + j;
 *   with nused < 2 every mean and every scat entry of the member is NaN.
 *
 * 2. pm_series_eof -- per unit u (q, n, nu, iters; nused and scat as entry 1 stored them):
 *   the members of u are taken in `order`; those with nused < 2 are skipped
 *   N        = the sum of their nused (int32), stored as ntot[u]
 *   P_ij     = the sum of their S_ij
 *   C_ij     = P_ij / (double)N for j <= i, C_ji = C_ij
 *   trace    = sum_i C_ii, stored as it is
 *   if N == 0, or trace is not finite, or trace <= 0: eof, lam, resid and vv are NaN.  Otherwise
 *   p0       = the first argmax of C_ii;  y_i = C_{i,p0}
 *   exactly `iters` times, a fixed count with no early exit, 1 <= iters <= PM_EOF_ITERS_MAX = 1024:
 *     p      = the first argmax of |y_i|
 *     if y_p is zero or not finite: eof, lam, resid and vv are NaN, and the iteration ends
 *     v_i    = y_i / y_p            (v_p is exactly 1: the sign is fixed, the largest loading is
 *                                    positive)
 *     y_i    = sum_j C_ij * v_j
 *   then once more p, the same test of y_p, v_i = y_i / y_p and y_i = sum_j C_ij * v_j, and
 *   vy       = sum_i v_i * y_i;  vv = sum_i v_i * v_i;  lam = vy / vv    (the Rayleigh quotient)
 *   resid    = (the first max over i of |y_i - lam * v_i|) / |lam|
 *   stores eof[q][nu] (= v), lam[nu], trace[nu], resid[nu], vv[nu], ntot[nu] (int32).
 *   resid is the caller's read-out of convergence: the iteration count is fixed so that a result is
 *   a pure function of its input, and whether `iters` sufficed shows in resid, not in the count
 *   (two equal leading eigenvalues give a deterministic result with a large resid).  lam / trace
 *   is the fraction of variance the mode holds.
 *
 * 3. pm_series_project -- per member m, u = unit[m] (m itself with unit NULL), per record k of the
 * window:
 *   pc[k][0][m] = sum_j ((x_kj - mean_jm) * w_jm) * eof_j[u]        for a used record
 *   NaN for an unused record, for nused[m] < 2 and wherever an eof_j[u] is NaN
 *   pc is a device series [K][1][n] that every pm_series_* entry reads as it stands.
 *   The EOF is normalised to a largest loading of 1, not to unit length (that would take a sqrt):
 *   pc is the unit-length component times the constant sqrt(vv).  ac, the DFA exponent, the
 *   restoring rate and Kendall's tau do not see the scale; var scales by vv, which entry 2 returns.
 * A result of entries 1 and 3 depends on that member's values (and its unit's EOF) alone: not on
 * n, the shard or the launch geometry.
 *
 * Checked before anything is launched (PM_EINVAL, outputs untouched): n, nspec, nrec >= 1 and
 * 0 <= k0 < k1 <= nrec (entries 1 and 3); K >= 2; q and iters in the ranges above; every sel in
 * [0, nspec) and no two equal; no NULL pointer but w, and order, start, start_dev and unit, which
 * are NULL together (entry 2: then nu = n; entry 3: unit NULL needs nu = n); 1 <= nu <= n; start[0]
 * = 0, start monotone, start[nu] = n, no unit larger than PM_STATS_GROUP_MAX; K < 2^30 and the
 * grids below 2^31 blocks.  The checks read the HOST mirror start; the kernel reads start_dev.
 * That order is a permutation and that unit agrees with it are the caller's to ensure.          */
#define PM_EOF_Q_MAX 32
#define PM_EOF_ITERS_MAX 1024
struct pm_series_scatter {
  int32_t n, nspec, nrec, k0, k1, q, reserved1, reserved2;
  const double *v;                       /* device [nrec][nspec][n]                               */
  const double *w;                       /* device [q][n], or NULL: 1.0                           */
  int32_t sel[PM_EOF_Q_MAX];             /* sel[j], j < q (the rest is not read)                  */
};
int pm_series_scatter(const struct pm_series_scatter *d, int32_t *nused, double *mean,
                      double *scat, pm_stream_t stream);
struct pm_series_eof {
  int32_t n, q, nu, iters;
  const int32_t *nused;                  /* device [n]                                            */
  const double *scat;                    /* device [q (q + 1) / 2][n]                             */
  const int32_t *order;                  /* device [n], or NULL: every member a unit              */
  const int32_t *start;                  /* HOST [nu + 1], or NULL                                */
  const int32_t *start_dev;              /* DEVICE, the same values, or NULL                      */
};
int pm_series_eof(const struct pm_series_eof *d, double *eof, double *lam, double *trace,
                  double *resid, double *vv, int32_t *ntot, pm_stream_t stream);
struct pm_series_project {
  int32_t n, nspec, nrec, k0, k1, q, nu, reserved;
  const double *v;                       /* device [nrec][nspec][n]                               */
  const double *w;                       /* device [q][n], or NULL: 1.0                           */
  const int32_t *nused;                  /* device [n]                                            */
  const double *mean;                    /* device [q][n]                                         */
  const double *eof;                     /* device [q][nu]                                        */
  const int32_t *unit;                   /* device [n], or NULL: unit[m] = m                      */
  int32_t sel[PM_EOF_Q_MAX];
};
int pm_series_project(const struct pm_series_project *d, double *pc, pm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PYMOC_HIP_H */
