/*
 * tmhpvsim.h — C-ABI of the MI355X batched simulator for tmhpvsim's
 * clear-sky-index chain + PV model (libtmhpvsim.so, gfx950).
 *
 * The reference (coroa/tmhpvsim) is pure Python; its per-step operator API is
 *   ClearskyindexModel(time).next(time) -> float   tmhpvsim/clearskyindexmodel.py:57,128
 *   PVModel(time).next(time) -> float              tmhpvsim/pvmodel.py:12,82
 *   get_meter_value() -> float                     tmhpvsim/metersim.py:49
 *   residual = meter - pv                          tmhpvsim/pvsim.py:83
 * The Python package tmhpvsim_amd keeps those classes and signatures and binds
 * this library with ctypes (tmhpvsim_amd/_lib.py); INTEGRATION.md shows the
 * ctypes stub a reference maintainer would add.  Every entry point below
 * replaces a batch of those per-step calls: one call advances N chains
 * (chain = site x scenario) over a window of consecutive seconds.
 *
 * Conventions
 *  - plain pointers and sizes only; every device buffer is allocated by the
 *    caller (PyTorch-ROCm in tmhpvsim_amd) and passed as a raw device pointer.
 *    The library allocates nothing persistent on the device.
 *  - return 0 on success or a negative TMH_E_* code; never aborts; the last
 *    error message of the calling thread is available from tmh_last_error().
 *  - model faults that the reference raises as Python exceptions are reported
 *    per chain in the state's status word (TMH_CHAIN_*); a faulted chain is
 *    frozen and emits NaN (covered = 255) from the faulting step on.
 *  - outputs of a window: per-second traces (tmh_trace), per-chain totals and a
 *    histogram (tmh_stats), the fleet series (tmh_series: per second, summed over
 *    the chains) and interval metering (tmh_intervals: per chain, summed over the
 *    seconds of each metering interval -- what a household's 15-minute or hourly
 *    meter reads; exact integer sums, compacted windows included) or, in its place,
 *    the import / export registers (tmh_registers: the intervals' columns plus what
 *    the chain drew from the grid and what it fed in, per interval) or the demand
 *    registers (tmh_demand: the registers' columns plus the peak import and the peak
 *    feed-in of each interval and the second of each) or battery storage (tmh_storage,
 *    fp64 engines: the intervals' columns plus what the meter reads with a battery behind
 *    it, what the battery took and gave and its state of charge at each interval's end) or
 *    the battery kind (tmh_battery: the same with charge and discharge efficiency, a standby
 *    drain, a loss column and per-chain battery parameters), and beside that kind's table the
 *    battery fleet series (tmh_set_battery_fleet: per second, summed over the chains, what the
 *    fleet draws, feeds in, stores and charges behind its batteries), or the battery sweep
 *    (tmh_battery_sweep: the battery kind's table and state of charge for each of up to
 *    TMH_BATTERY_SWEEP_MAX candidate batteries per chain, in one run), or battery dispatch
 *    (tmh_dispatch: the battery kind with a charge threshold, a discharge threshold and a
 *    feed-in limit per chain, the curtailed energy and the peaks behind the battery), or the
 *    dispatch sweep (tmh_dispatch_sweep: battery dispatch's table and state of charge for each
 *    of up to TMH_DISPATCH_SWEEP_MAX rule sets per chain, in one run), or scheduled dispatch
 *    (tmh_schedule: battery dispatch with up to TMH_SCHEDULE_RULES_MAX rule sets per chain, one
 *    of them in force per metering interval, and charging from the grid), or the schedule sweep
 *    (tmh_schedule_sweep: scheduled dispatch's table and state of charge for each of up to
 *    TMH_SCHEDULE_SWEEP_MAX variants -- battery, rule sets and rule array -- per chain, in one run).
 *  - `stream` is a hipStream_t (NULL = default stream); all work is enqueued
 *    asynchronously on it.  One engine per device; not re-entrant per engine.
 */
#ifndef TMHPVSIM_H
#define TMHPVSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMH_ABI_VERSION 1

/* ---- error codes ---- */
#define TMH_OK 0
#define TMH_E_INVAL (-1)
#define TMH_E_HIP (-2)
#define TMH_E_NOMEM (-3)
#define TMH_E_STATE (-4)

/* ---- per-chain status (the reference's exceptions) ---- */
#define TMH_CHAIN_OK 0
#define TMH_CHAIN_NAMEERROR_INIT 1  /* clearskyindexmodel.py:72-80 (undefined x, cc in [0.75,0.875)) */
#define TMH_CHAIN_ASSERT_BINARY 2   /* cloud_cover_binary.py:90-98 (assert not recurse) */
#define TMH_CHAIN_SIGMA_OVERFLOW 3  /* sigma arrays exceed TMH_SIGMA_CAP (no reference analogue) */
#define TMH_CHAIN_U_EXHAUSTED 4     /* injected uniform stream ran out */
#define TMH_CHAIN_SEGMENT_OVERFLOW 5 /* more than cap + 2,048 cloud segments in one window, where the row
                                         cap = (n_steps/135 + 16) rounded up to 16 (656 a day: ~1.7x the
                                         mean 386 calls, exceeded by ~0.3 % of the chain-days); or more
                                         than cap while the batch's demand exceeds the window's shared
                                         overflow pool (n/16 + 8 chunks of 256): then every such chain
                                         faults at its first record past the row (deterministic;
                                         time-parallel path) */
#define TMH_CHAIN_GUARD_OVERFLOW 6   /* fp32 guard-band records of the batch exceeded their room (never observed; time-parallel path) */

/* ---- modes ---- */
#define TMH_CC_FAITHFUL 0  /* reference: a fresh get_cloud_cover generator per hourly draw */
#define TMH_CC_MARKOV 1    /* persistent 6-bin hourly Markov chain (cloud_cover_hourly.py:290-316) */
#define TMH_RNG_KEYED 0    /* counter-based Philox4x32-10 keyed by (chain, step, draw family) */
#define TMH_RNG_INJECTED 1 /* per-chain uniform stream, consumed in reference order */
#define TMH_FP32 0         /* per-second CSI/PV/meter arithmetic in fp32 (Markov state stays fp64) */
#define TMH_FP64 1         /* everything in fp64 */
#define TMH_PATH_AUTO 0          /* time-parallel when possible (keyed + faithful), else sequential */
#define TMH_PATH_SEQUENTIAL 1    /* one work-item per chain, seconds in order */
#define TMH_PATH_TIME_PARALLEL 2 /* segment pass + (chain x 128 s block) expansion */

#define TMH_SIGMA_CAP 512  /* capacity of sigma_cloud / sigma_clear per chain (max seen: 132) */
#define TMH_GEOM_FIELDS 22 /* doubles per step in the clock/geometry table (DESIGN.md "Data layout") */

/* ---- SAPM module parameter order (tmh_params.module) ---- */
enum {
    TMH_MOD_A0 = 0, TMH_MOD_A4 = 4, TMH_MOD_B0 = 5, TMH_MOD_B5 = 10, TMH_MOD_FD = 11,
    TMH_MOD_IMPO = 12, TMH_MOD_VMPO = 13, TMH_MOD_AIMP = 14, TMH_MOD_C0 = 15, TMH_MOD_C1 = 16,
    TMH_MOD_C2 = 17, TMH_MOD_C3 = 18, TMH_MOD_BVMPO = 19, TMH_MOD_MBVMP = 20, TMH_MOD_N = 21,
    TMH_MOD_NS = 22, TMH_MOD_TEMP_A = 23, TMH_MOD_TEMP_B = 24, TMH_MOD_TEMP_DT = 25,
    TMH_MOD_COUNT = 26
};
/* ---- Sandia inverter order (tmh_params.inverter): Paco Pdco Vdco Pso C0 C1 C2 C3 Pnt ---- */
#define TMH_INV_COUNT 9

typedef struct tmh_params {
    int32_t cc_mode;          /* TMH_CC_* */
    int32_t rng_mode;         /* TMH_RNG_* */
    int32_t precision;        /* TMH_FP32 / TMH_FP64 */
    int32_t with_pv;          /* 0: pv = 0 (CSI-only runs, as ClearskyindexModel) */
    int32_t kernel_path;      /* TMH_PATH_* */
    int32_t reserved;
    uint64_t seed;            /* keyed Philox seed (the meter always draws keyed) */
    double shapes[6][4];      /* loc, scale, kappa, df per cloud-cover bin (mc_dist_shapes.csv) */
    int32_t shape_is_t[6];    /* 1: Student-t bin, 0: asymmetric Laplace */
    double edges[6];          /* right edges of the bins */
    double site[8];           /* lat, lon, altitude, tilt, surface azimuth, albedo, temp_air, wind */
    double linke[12];         /* monthly Linke turbidity */
    double module[TMH_MOD_COUNT];
    double inverter[TMH_INV_COUNT];
} tmh_params;

/* Wall clock of a run.  Step s is the (s+1)-th call of ClearskyindexModel.next;
 * the engine is constructed at the time of step 0 (clearskyindexmodel.py:57). */
typedef struct tmh_clock {
    int64_t utc0;            /* unix seconds of step 0 (solar geometry) */
    int64_t local0;          /* local wall-clock seconds of step 0, counted from 1970-01-01 00:00 local */
    int32_t n_shifts;        /* DST changes within the horizon (<= 8) */
    int32_t reserved;
    int64_t shift_step[8];   /* from this step on ... */
    int32_t shift_delta[8];  /* ... local time is shifted by this many seconds (e.g. -3600) */
} tmh_clock;

/* Injected uniform streams: chain i (0-based within the call) reads
 * u[i * stride + k] for its k-th draw, k < len.  Device pointer. */
typedef struct tmh_ustream {
    const double* u;
    uint64_t stride;
    uint64_t len;
} tmh_ustream;

/* Per-second traces, time-major: element (step j of the call, chain i) lives at
 * [j * ld + i].  Real = float (TMH_FP32) or double (TMH_FP64).  Any may be NULL. */
typedef struct tmh_trace {
    void* csi;          /* clear-sky index (ClearskyindexModel.next) */
    uint8_t* covered;   /* CloudCoverBinary bit (1 = the "covered" branch), 255 on fault */
    void* pv;           /* AC power, W (PVModel.next) */
    void* meter;        /* 9000 * U, W (get_meter_value) */
    void* residual;     /* meter - pv, W (pvsim.py:83) */
    uint64_t ld;        /* >= n_chains */
} tmh_trace;

/* On-GPU statistics, accumulated over calls (caller zero-initialises).  Device pointers. */
typedef struct tmh_stats {
    uint64_t* hist;     /* [n_bins] residual histogram, edge bins absorb out-of-range; NULL = off */
    uint32_t n_bins;
    uint32_t reserved;
    double lo, hi;      /* histogram range, W */
    double* chain_acc;  /* [4][n_chains] sum pv, sum meter, sum residual (W*s), max residual */
} tmh_stats;

/* Fleet series: exact per-second sums over the chains of a group, accumulated over
 * calls (caller zero-initialises).  sum: device int64 [n_groups][n_steps][4]; row s of a
 * group holds, for step step0 + s, over the group's chains that are ok at that step
 * (live and before their fault):
 *   [0] sum of q(pv)   [1] sum of q(meter)   [2] n_ok   [3] ok chains with the covered bit
 * with q(v) = v * 2^TMH_SERIES_FRAC_BITS rounded half to even to an integer, v the engine's
 * final value (fp32 engines: the fp32 value a trace would hold after the guard-band fixup;
 * fp64 engines: the fp64 value).  Residual = [1] - [0].  Integer sums: the bits do not
 * depend on block, wave, window, batch or shard order.  Chain i of a call belongs to
 * group i / group_chains (0: one group; else a multiple of 512).  A faulted chain's
 * seconds before its fault count; a chain faulted at construction adds nothing. */
#define TMH_SERIES_FRAC_BITS 12        /* q in units of 2^-12 W */
#define TMH_SERIES_MAX_W 16384.0       /* |pv|, |meter| < 2^14 W: 32 lanes x 2^26 fit an int32 partial */
typedef struct tmh_series {
    int64_t* sum;
    int64_t step0;
    uint32_t n_steps, group_chains, n_groups, reserved;
} tmh_series;

/* Interval metering: what each chain's interval meter reads -- exact per-chain sums per
 * metering interval (15 minutes, an hour, any number of seconds), accumulated over calls
 * (the caller zero-initialises).  sum: device int64 [n_intervals][4][ld]; cell (k, col, i)
 * sits at sum[(k*4 + col)*ld + i] and holds, over the seconds of interval k (steps
 * [step0 + k*interval_s, step0 + (k+1)*interval_s), cut at step0 + n_steps) at which chain
 * i is ok (live and before its fault):
 *   [0] sum of q(pv)   [1] sum of q(meter)   [2] ok seconds   [3] ok seconds with the covered bit
 * with the fleet series' q and TMH_SERIES_FRAC_BITS (the engine's final value -- fp32
 * engines: after the guard-band fixup -- rounded half to even); residual energy is
 * [1] - [0].  i is the chain's index in the batch (under tmh_set_chain_ids: ids[slot], as
 * tmh_stats.chain_acc), so compacted windows fill the same table.  Integer sums: the bits
 * do not depend on block, wave, window, batch, compaction or launch order.  A chain
 * faulted at construction adds nothing; one that faults inside an interval keeps its
 * seconds before the fault. */
typedef struct tmh_intervals {
    int64_t* sum;        /* device int64 [n_intervals][4][ld], accumulated; the caller zero-initialises */
    int64_t step0;       /* origin: step s belongs to interval (s - step0) / interval_s */
    uint32_t n_steps;    /* steps covered; n_intervals = ceil(n_steps / interval_s); a last partial interval is kept */
    uint32_t interval_s; /* >= 1, any value (60, 900 and 3600 are the usual ones) */
    uint64_t ld;         /* >= the batch's chains (>= n_full under tmh_set_chain_ids) */
} tmh_intervals;

/* Import / export registers: the two registers of a household's bidirectional meter (OBIS
 * 1.8.0 / 2.8.0) beside the interval meter's columns -- how much each chain drew from the
 * grid and how much it fed in, per metering interval.  Both are non-linear per second, so
 * no other table gives them.  sum: device int64 [n_intervals][TMH_REGISTERS_COLS][ld],
 * accumulated (the caller zero-initialises); cell (k, col, i) sits at sum[(k*6 + col)*ld + i].
 * Columns 0-3 are tmh_intervals' (same q, TMH_SERIES_FRAC_BITS, ok rule, chain index and
 * partial last interval); over the same ok seconds
 *   [4] import = sum of max(q(meter) - q(pv), 0)   [5] export = sum of max(q(pv) - q(meter), 0)
 * on the quantised integers (|q| < 2^26: a second's difference fits an int32), so for
 * every cell [4] - [5] == [1] - [0] bit for bit, and the self-consumed energy is
 * [0] - [5] == [1] - [4].  Integer sums, as the intervals'. */
#define TMH_REGISTERS_COLS 6
typedef struct tmh_intervals tmh_registers;   /* the same descriptor: sum is [n_intervals][6][ld] */

/* Demand registers: a meter's maximum-demand registers beside the import / export registers
 * -- per chain and metering interval, the highest power drawn from the grid and the highest
 * power fed in, and when each happened (what sizing a feeder, a transformer or an inverter
 * asks for; a maximum is non-linear, so no other table gives it).  sum: device int64
 * [n_intervals][TMH_DEMAND_COLS][ld]; cell (k, col, i) sits at sum[(k*8 + col)*ld + i]; the
 * caller zero-initialises.  Columns 0-5 are tmh_registers' exactly (same q,
 * TMH_SERIES_FRAC_BITS, ok rule, chain index, partial last interval and identity
 * [4] - [5] == [1] - [0]).  Columns 6 and 7 are packed keys combined by maximum, within a call
 * and across calls: for an ok second s of interval k, o = s - step0 - k * interval_s and
 *   key(v, o) = (v << 32) | (0xFFFFFFFF - o)
 *   [6] peak import: v = max(q(meter) - q(pv), 0)   [7] peak export: v = max(q(pv) - q(meter), 0)
 * on the quantised integers (fp32 engines: the value after the fixup).  The cell is the
 * maximum key over the interval's ok seconds: its high word is the peak in units of
 * 2^-TMH_SERIES_FRAC_BITS W, its low word gives the earliest second at which it occurred
 * (o = 0xFFFFFFFF - low word).  v < 2^27 and o < interval_s <= 2^32 - 1, so every ok second's
 * key is positive (signed and unsigned maxima agree) and 0 means "no ok second": zero is the
 * identity of the maximum.  An interval without feed-in has [7] = key(0, its first ok second):
 * one rule, no special cases. */
#define TMH_DEMAND_COLS 8
typedef struct tmh_intervals tmh_demand;      /* the same descriptor: sum is [n_intervals][8][ld], accumulated / maximised */

/* Battery storage: a battery behind each chain's meter, charged from the PV surplus and
 * discharged into the deficit (greedy self-consumption, lossless), and what the meter reads
 * with it.  The state of charge (SoC) depends on every earlier second of the chain, so no
 * other table can be post-processed into this one.  All quantities are integers in the
 * series' units: powers in 2^-TMH_SERIES_FRAC_BITS W, energies and SoC in 2^-12 W s.
 * capacity C (0 <= C < 2^40), p_charge Pc and p_discharge Pd (0 .. 2^27 each) are uniform
 * over the batch; soc[i] is chain i's SoC x (i as tmh_intervals': ids[slot] under
 * tmh_set_chain_ids), read at a window's start and written at its end.  For an ok second
 * with d = q(pv) - q(meter):
 *   a  = clamp(d, -Pd, Pc)      what the battery is asked to take (+) or give (-)
 *   x' = clamp(x + a, 0, C)     (64-bit)
 *   g  = x' - x                 what it took / gave
 *   import_b = max(g - d, 0)    export_b = max(d - g, 0)
 * A second that is not ok leaves x unchanged (a faulted or dead chain's battery holds its
 * charge).  The initial x is taken as given; after the first ok second it lies in [0, C].
 * table.sum: device int64 [n_intervals][TMH_STORAGE_COLS][ld], cell (k, col, i) at
 * sum[(k*9 + col)*ld + i], zero-initialised by the caller.  Over the ok seconds of interval k:
 *   [0..3] tmh_intervals' columns exactly          (added)
 *   [4] sum of import_b   [5] sum of export_b      (added)
 *   [6] sum of max(g, 0)  [7] sum of max(-g, 0)    (added: charged, discharged)
 *   [8] the maximum of ((o + 1) << 40) | x'        (o: the second's offset in its interval)
 * so [8] is the key of the interval's last ok second: its low 40 bits are the SoC at the end
 * of the interval (or at the chain's fault); 0: no ok second.  Keys are positive and 0 is the
 * identity of the maximum; interval_s <= 2^23 - 1.  For every cell [4] - [5] == [1] - [0] +
 * [6] - [7], columns 4-7 are >= 0, and [6] - [7] is the interval's SoC change.  With C = 0 or
 * Pc = Pd = 0 columns 4 and 5 are tmh_registers'.  The bits do not depend on windows,
 * batches, shards or compaction and equal a sequential loop over the traces.
 * fp64 engines only: an fp32 engine replaces its guard-band seconds after the expansion
 * (fixup_kernel) -- an additive correction for a sum, but a changed second changes the SoC of
 * every later second, so the expansion would need the fixed values before it runs.
 * work: device scratch of the caller, >= tmh_storage_work_bytes(n_chains, n_steps) bytes for
 * the largest window (three int64 per chain and 128-step block), 8-byte aligned; its
 * contents mean nothing between calls. */
#define TMH_STORAGE_COLS 9
typedef struct tmh_storage {
    tmh_intervals table;      /* sum is [n_intervals][9][ld] */
    int64_t* soc;             /* device [ld]: per chain index, read at a window's start, written at its end */
    void* work;               /* device scratch */
    size_t work_bytes;        /* >= tmh_storage_work_bytes(n_chains, n_steps) of the largest window */
    int64_t capacity, p_charge, p_discharge;
} tmh_storage;

/* The battery kind: tmh_storage's battery with charge and discharge efficiency, a standby
 * drain and per-chain parameters.  tmh_storage stays as it is (lossless, uniform); this kind
 * reproduces it bit for bit in columns 0-8 and soc when every chain has ec = ed = 2^16 and
 * sigma = 0, and its column 9 is then 0.  Integers in the series' units as above.
 * params: device int64 [6][ld] of the caller (ld: table.ld), row r of chain i at
 * params[r*ld + i], i as soc's (ids[slot] under tmh_set_chain_ids); a column slice of a
 * larger [6][N] tensor is a valid argument.  Read by every window, never written:
 *   row 0  capacity C                                0 <= C < 2^40
 *   row 1  charge limit Pc at the meter side         0 .. 2^27
 *   row 2  discharge limit Pd at the meter side      0 .. 2^27
 *   row 3  charge efficiency ec in 2^-16             2^15 .. 2^16
 *   row 4  discharge efficiency ed in 2^-16          2^15 .. 2^16
 *   row 5  standby drain sigma per ok second         0 .. 2^27
 * No address depends on a parameter; a value outside its range is clamped into it when a lane
 * loads it, so the result is defined without the host reading the tensor.  Two multipliers are
 * derived: kc = ceil(2^32 / ec), kd = ceil(2^32 / ed) (= floor((2^32 - 1) / e) + 1; in
 * [2^16, 2^17]).  The SoC x is clamped into [0, C] when a window reads it; at a window's end
 * it lies there, so splitting into windows changes nothing.  For an ok second with
 * d = q(pv) - q(meter) and the SoC x before it:
 *   a  = clamp(d, -Pd, Pc)                                   asked at the meter side
 *   s  = a >= 0 ?  (a*ec) >> 16  :  -((-a*kd + 65535) >> 16) stored (floor) / drained (ceil)
 *   x1 = clamp(x + s, 0, C)          g = x1 - x
 *   b  = a                                    if g == s      (not clipped)
 *      =  min( a, (g*kc + 65535) >> 16)       if g > 0       (fills during this second)
 *      = -min(-a, (-g*ed) >> 16)              if g < 0       (runs empty during this second)
 *      = 0                                    if g == 0
 *   x' = max(x1 - sigma, 0)
 *   import_b = max(b - d, 0)   export_b = max(d - b, 0)   loss = b - (x' - x)
 * A second that is not ok leaves x unchanged and adds nothing.  All products stay below 2^60;
 * loss >= 0, |b| <= |a| and b has a's sign in every second.  The second's map of x is the
 * clamped addition {s, 0, C} followed by {-sigma, 0, C}: tmh_storage's algebra and its three
 * launches carry over.
 * table.sum: device int64 [n_intervals][TMH_BATTERY_COLS][ld], zero-initialised by the caller.
 * Over the ok seconds of interval k:
 *   [0..3] tmh_intervals' columns exactly            (added)
 *   [4] sum of import_b    [5] sum of export_b       (added)
 *   [6] sum of max(b, 0)   [7] sum of max(-b, 0)     (added: charged, discharged, meter side)
 *   [8] the maximum of ((o + 1) << 40) | x'          (tmh_storage's key)
 *   [9] sum of loss                                  (added)
 * For every cell [4] - [5] == [1] - [0] + [6] - [7], columns 4-7 and 9 are >= 0, and
 * [6] - [7] - [9] is the interval's SoC change.  The bits do not depend on windows, batches,
 * shards or compaction and equal a sequential loop over the traces.  fp64 engines only, as
 * tmh_storage.  soc, work and work_bytes: tmh_storage's (tmh_storage_work_bytes). */
#define TMH_BATTERY_COLS 10
typedef struct tmh_battery {
    tmh_intervals table;      /* sum is [n_intervals][10][ld] */
    int64_t* soc;             /* device [ld]: per chain index, read (clamped into [0, C]) at a window's start, written at its end */
    void* work;               /* device scratch */
    size_t work_bytes;        /* >= tmh_storage_work_bytes(n_chains, n_steps) of the largest window */
    const int64_t* params;    /* device [6][ld], ld = table.ld */
} tmh_battery;

/* The battery fleet series: the fleet series behind the batteries -- what the whole batch draws from
 * the grid and feeds in second by second once the battery kind's batteries are in, and the energy the
 * fleet holds at that second.  An output of the battery kind beside its interval table (never instead
 * of it): the replay pass has every quantity of tmh_battery's per-second rule in a register and reduces
 * it across the chains.  The descriptor is tmh_series with TMH_BATTERY_FLEET_COLS columns per row:
 * sum is device int64 [n_groups][n_steps][8], accumulated over calls (the caller zero-initialises);
 * row s of a group holds, for step step0 + s, over the group's chains that are ok at that step (the
 * fleet series' rule and groups: chain i of a call in group i / group_chains, 0: one group, else a
 * multiple of 512):
 *   [0] sum of q(pv)   [1] sum of q(meter)   [2] n_ok   [3] ok chains with the covered bit
 *       -- tmh_series' four columns, bit for bit what tmh_set_series gives for the same chains
 *   [4] sum of import_b     what the fleet draws from the grid behind its batteries
 *   [5] sum of export_b     what it feeds in
 *   [6] sum of x'           the state of charge after the second, in 2^-12 W s
 *   [7] sum of max(b, 0)    what the batteries take at the meter side
 * with import_b, export_b, b and x' exactly tmh_battery's.  For every row [4] - [5] == [1] - [0] + sum
 * of b, so the fleet's net battery power follows from the row and the discharging power is [7] - sum
 * of b; columns 4-7 are >= 0; [6] <= the sum of C over the group.  A chain that is not ok at a second
 * (faulted, or dead from construction) adds nothing to that row, its stored energy included.
 * Bounds: b lies between 0 and d, so per chain export_b <= max(d, 0) <= q(pv) and max(b, 0) <= q(pv),
 * below 2^26, and import_b <= max(-d, 0) <= q(meter) (+ |q(pv)| in a daylight second whose pv is the
 * inverter's night tare), below 2^27: 32 lanes of each fit a 32-bit partial (the three are >= 0 and
 * summed unsigned); x' < 2^40 does not and is reduced as two 20-bit halves (32 x 2^20 each).  Integer
 * sums: the bits do not depend on block, wave, window, batch or pipelining order and equal a
 * sequential loop over the traces. */
#define TMH_BATTERY_FLEET_COLS 8

/* The battery sweep: tmh_battery's rule, unchanged to the bit, applied to n_variants parameter sets
 * per chain in one run -- the same household (the same chain: the same pv and meter second for
 * second) behind each of K candidate batteries.  Variant v has a table, a state of charge and
 * parameters of its own, each exactly what tmh_set_battery would be given and would produce for it:
 *   table.sum  device int64 [n_variants][n_intervals][TMH_BATTERY_COLS][ld], zero-initialised by the
 *              caller; variant v's table starts n_intervals * TMH_BATTERY_COLS * ld elements after
 *              variant v - 1's (n_intervals = ceil(table.n_steps / table.interval_s)) and equals
 *              tmh_battery's table for params[v] and soc[v] bit for bit, so columns 0-3 are the
 *              same in every variant
 *   soc        device int64 [n_variants][ld]: variant v's row at soc + v * ld, tmh_battery's soc
 *   params     device int64 [n_variants][6][ld]: variant v's six rows at params + v * 6 * ld, rows,
 *              ranges and clamping as tmh_battery's; read by every window, never written
 * Indexing within a variant is per chain index (ids[slot] under tmh_set_chain_ids), so compacted
 * windows fill the same tables; the strides are in units of ld, so a column slice of wider tensors
 * ([K][n_iv][10][N], [K][6][N], [K][N] with ld = N) is a valid argument, as it is for tmh_battery.
 * work: device scratch of the caller, >= tmh_battery_sweep_work_bytes(n_chains, n_steps, n_variants)
 * = n_variants * tmh_storage_work_bytes(n_chains, n_steps) bytes of the largest window.  The engine
 * runs the variants in groups of a compile-time count per launch (the kind's three launches per
 * group); the bits do not depend on the grouping, windows, batches or compaction.  fp64 engines and
 * the engine's one site only. */
#define TMH_BATTERY_SWEEP_MAX 16
typedef struct tmh_battery_sweep {
    tmh_intervals table;      /* sum is [n_variants][n_intervals][TMH_BATTERY_COLS][ld] */
    int64_t* soc;             /* device [n_variants][ld] */
    void* work;               /* device scratch */
    size_t work_bytes;        /* >= tmh_battery_sweep_work_bytes(n_chains, n_steps, n_variants) of the largest window */
    const int64_t* params;    /* device [n_variants][6][ld], rows as tmh_battery's */
    uint32_t n_variants;      /* 1 .. TMH_BATTERY_SWEEP_MAX */
} tmh_battery_sweep;

/* Battery dispatch: the battery kind (tmh_battery above) under another control rule than greedy
 * self-consumption.  The battery charges only from the surplus above a threshold, discharges only into the
 * deficit above a threshold, and what is left of the surplus is fed in up to a limit, the rest curtailed.
 * tmh_battery stays as it is; this kind reproduces it bit for bit in columns 0-9 and soc when every chain has
 * Tc = Td = 0 and L = 2^27, and its column 10 is then 0.  Integers in the series' units as above.
 * params: device int64 [9][ld] of the caller, laid out and read as tmh_battery's; rows 0-5 are tmh_battery's
 * exactly (C, Pc, Pd, ec, ed, sigma), then
 *   row 6  charge threshold Tc: the battery charges only from the surplus above it       0 .. 2^27
 *   row 7  discharge threshold Td: it discharges only into the deficit above it          0 .. 2^27
 *   row 8  feed-in limit L; 2^27 means none, since a second's surplus stays below 2^26    0 .. 2^27
 * each read per chain and clamped into its range as a lane loads it; no address depends on a value.  For an
 * ok second with d = q(pv) - q(meter) and the SoC x before it:
 *   a  = d >= 0 ?  min(max(d - Tc, 0), Pc)  :  -min(max(-d - Td, 0), Pd)       asked at the meter side
 *   s, x1, g, b, x'   exactly tmh_battery's rule applied to this a
 *   r  = d - b                      what is left at the meter (b lies between 0 and d: r has d's sign or is 0)
 *   import_b  = max(-r, 0)          surplus = max(r, 0)
 *   export_b  = min(surplus, L)     fed in
 *   curtailed = surplus - export_b  what the inverter throws away
 *   loss      = b - (x' - x)
 * A second that is not ok leaves x unchanged and adds nothing.  The ask depends on d and the chain's constants
 * only, so the second's map of x is tmh_battery's pair of clamped additions: its three launches carry over.
 * table.sum: device int64 [n_intervals][TMH_DISPATCH_COLS][ld], zero-initialised by the caller.
 * Over the ok seconds of interval k:
 *   [0..3] tmh_intervals' columns exactly            (added; [0] stays the available PV: produced = [0] - [10])
 *   [4] sum of import_b    [5] sum of export_b       (added; export_b after the limit)
 *   [6] sum of max(b, 0)   [7] sum of max(-b, 0)     (added)
 *   [8] tmh_storage's SoC key                        (maximum)
 *   [9] sum of loss        [10] sum of curtailed     (added)
 *   [11] peak import behind the battery: the maximum of tmh_demand's key (v << 32) | (0xFFFFFFFF - o), v = import_b
 *   [12] peak feed-in: the same key with v = export_b
 * [11] and [12]: 0 means no ok second; an interval without feed-in holds key(0, its first ok second), as
 * tmh_demand.  For every cell [4] - [5] == [1] - [0] + [6] - [7] + [10], columns 4-7, 9 and 10 are >= 0,
 * [6] - [7] - [9] is the interval's SoC change and the peak in [12] is <= L.  Reductions: with Tc = Td = 0 and
 * L = 2^27, columns 0-9 and soc are tmh_set_battery's bit for bit and column 10 is 0; with C = 0 and L = 2^27,
 * columns 11 and 12 are the fp64 demand kind's columns 6 and 7; with C = 0 and any L, [5] + [10] is the
 * registers' export.  (The two C = 0 reductions are exact for ec = 2^16.  With ec < 2^16 an ask of exactly one
 * unit stores s = 0, so g == s and tmh_battery's rule gives b = a = 1: that unit is taken from the surplus and
 * lost, in this kind as in tmh_battery, so such a second's export_b is one unit below the registers'.)  The bits do not depend on windows, pipelining, batches, column slices or compaction and
 * equal a sequential loop over the traces.  fp64 engines only, as tmh_battery.  soc, work and work_bytes:
 * tmh_battery's (tmh_storage_work_bytes). */
#define TMH_DISPATCH_COLS 13
#define TMH_DISPATCH_PARAMS 9
typedef struct tmh_dispatch {
    tmh_intervals table;      /* sum is [n_intervals][13][ld] */
    int64_t* soc;             /* device [ld]: as tmh_battery's */
    void* work;               /* device scratch */
    size_t work_bytes;        /* >= tmh_storage_work_bytes(n_chains, n_steps) of the largest window */
    const int64_t* params;    /* device [9][ld], ld = table.ld */
} tmh_dispatch;

/* The dispatch sweep: tmh_dispatch's rule, unchanged to the bit, applied to n_variants parameter sets per
 * chain in one run -- the same household (the same chain: the same pv and meter second for second) under each
 * of K rules and batteries: what a 70 % or a 60 % feed-in limit costs it, which charge threshold recovers the
 * curtailed energy, which battery to buy under the limit.  It relates to tmh_dispatch as tmh_battery_sweep
 * relates to tmh_battery.  Variant v has a table, a state of charge and parameters of its own, each exactly
 * what tmh_set_dispatch would be given and would produce for it:
 *   table.sum  device int64 [n_variants][n_intervals][TMH_DISPATCH_COLS][ld], zero-initialised by the caller;
 *              variant v's table starts n_intervals * TMH_DISPATCH_COLS * ld elements after variant v - 1's
 *              (n_intervals = ceil(table.n_steps / table.interval_s)) and equals tmh_dispatch's table for
 *              params[v] and soc[v] bit for bit, so columns 0-3 are the same in every variant
 *   soc        device int64 [n_variants][ld]: variant v's row at soc + v * ld, tmh_dispatch's soc
 *   params     device int64 [n_variants][TMH_DISPATCH_PARAMS][ld]: variant v's nine rows at params + v * 9 * ld,
 *              rows, ranges and clamping as tmh_dispatch's; read by every window, never written
 * Indexing within a variant is per chain index (ids[slot] under tmh_set_chain_ids), so compacted windows fill
 * the same tables; the strides are in units of ld, so a column slice of wider tensors ([K][n_iv][13][N],
 * [K][9][N], [K][N] with ld = N) is a valid argument.  work: device scratch of the caller, the battery sweep's:
 * >= tmh_battery_sweep_work_bytes(n_chains, n_steps, n_variants) bytes of the largest window.  The engine runs
 * the variants in groups of a compile-time count per launch (the kind's three launches per group; a group of
 * one variant is tmh_dispatch's own launches); the bits do not depend on the grouping, windows, batches or
 * compaction.  fp64 engines and the engine's one site only. */
#define TMH_DISPATCH_SWEEP_MAX 16
typedef struct tmh_dispatch_sweep {
    tmh_intervals table;      /* sum is [n_variants][n_intervals][TMH_DISPATCH_COLS][ld] */
    int64_t* soc;             /* device [n_variants][ld] */
    void* work;               /* device scratch */
    size_t work_bytes;        /* >= tmh_battery_sweep_work_bytes(n_chains, n_steps, n_variants) of the largest window */
    const int64_t* params;    /* device [n_variants][TMH_DISPATCH_PARAMS][ld], rows as tmh_dispatch's */
    uint32_t n_variants;      /* 1 .. TMH_DISPATCH_SWEEP_MAX */
} tmh_dispatch_sweep;

/* Scheduled dispatch: battery dispatch (tmh_dispatch above) whose rule changes at known times -- a time-of-use
 * tariff (discharge only in the expensive hours), charging from the grid in the cheap hours, delayed charging
 * under a feed-in limit, a controller that picks the thresholds per quarter hour.  A chain has one battery and
 * n_rules rule sets; one array shared by all chains of the engine says which rule is in force in each metering
 * interval of the table.  tmh_dispatch stays as it is; this kind reproduces it bit for bit (all thirteen columns
 * and soc) when no rule charges from the grid and the chain's rules are equal, when n_rules = 1, and when the
 * array names one rule throughout.  Integers in the series' units as above.
 * params: device int64 [6 + 4 * n_rules][ld] of the caller, laid out and read as tmh_dispatch's (row stride ld,
 * indexed per chain: ids[slot] under tmh_set_chain_ids; a column slice of a wider tensor is valid).  Rows 0-5 are
 * tmh_battery's exactly (C, Pc, Pd, ec, ed, sigma), constant over the run; rows 6 + 4r .. 9 + 4r are rule r's
 *   Tc  charge threshold       0 .. 2^27      Td  discharge threshold                      0 .. 2^27
 *   L   feed-in limit, 2^27 = none            G   grid-charge power, 0 = none              0 .. 2^27
 * each clamped into its range as a lane loads it.  A "hold" rule is Tc = Td = 2^27.
 * rule_of_interval: device uint8 [n_intervals], n_intervals = ceil(table.n_steps / table.interval_s): entry k is
 * the rule of the table's interval k, on the table's own grid and origin -- the index a window's step j has as
 * (step0 + j - table.step0) / interval_s.  Read by every window, never written; the kernels use min(entry,
 * n_rules - 1), so no address depends on an unchecked value.  Per-chain behaviour lives in the rule parameters (a
 * chain without a tariff gives all its rules the same values), not in the array.
 * An ok second in interval k, with (Tc, Td, L, G) the chain's rule rule_of_interval[k], d = q(pv) - q(meter) and
 * the SoC x before it:
 *   a0 = tmh_dispatch's ask: d >= 0 ? min(max(d - Tc, 0), Pc) : -min(max(-d - Td, 0), Pd)
 *   a  = G == 0 ? a0 : min(max(a0, 0) + G, Pc)            a grid-charging rule never discharges
 *   s, x1, g, b, x', r = d - b, import_b, export_b = min(max(r, 0), L), curtailed, loss: tmh_dispatch's on this a
 * With G > 0, b may exceed max(d, 0): the difference is bought from the grid and is part of import_b (< 2^26 +
 * 2^27).  |a| <= max(Pc, Pd) as before and the ask depends on d, the chain's constants and the time only, never
 * on x: the second is still tmh_battery's pair of clamped additions and the three launches carry over.
 * table.sum: device int64 [n_intervals][TMH_DISPATCH_COLS][ld], zero-initialised by the caller: tmh_dispatch's
 * thirteen columns with the same meanings.  For every cell [4] - [5] == [1] - [0] + [6] - [7] + [10], columns 4-7,
 * 9 and 10 are >= 0, [6] - [7] - [9] is the interval's SoC change and the peak in [12] is <= the L of the
 * interval's rule.  The bits do not depend on windows, pipelining, batches, column slices or compaction and equal
 * a sequential loop over the traces.  fp64 engines and the engine's one site only.  soc, work and work_bytes:
 * tmh_dispatch's (tmh_storage_work_bytes). */
#define TMH_SCHEDULE_RULES_MAX 8
#define TMH_SCHEDULE_RULE_PARAMS 4
typedef struct tmh_schedule {
    tmh_intervals table;      /* sum is [n_intervals][13][ld] */
    int64_t* soc;             /* device [ld]: as tmh_battery's */
    void* work;               /* device scratch */
    size_t work_bytes;        /* >= tmh_storage_work_bytes(n_chains, n_steps) of the largest window */
    const int64_t* params;    /* device [6 + 4 * n_rules][ld], ld = table.ld */
    const uint8_t* rule_of_interval;   /* device [n_intervals] */
    uint32_t n_rules;         /* 1 .. TMH_SCHEDULE_RULES_MAX */
} tmh_schedule;

/* The schedule sweep: tmh_schedule's second, unchanged to the bit, on n_variants (battery, rule sets, rule array)
 * variants of the same chain in one run -- the same household (the same pv and meter second for second) under each
 * of K tariffs and batteries: which tariff to take, whether grid charging at night pays under tariff A or B, which
 * battery to buy under it.  It relates to tmh_schedule as tmh_dispatch_sweep relates to tmh_dispatch.  Variant v's
 * slice of table, soc, params and rule_of_interval is exactly what tmh_set_schedule would be given and would
 * produce for it, all thirteen columns and soc bit for bit, so columns 0-3 are the same in every variant:
 *   table.sum         device int64 [n_variants][n_intervals][TMH_DISPATCH_COLS][ld], zero-initialised by the
 *                     caller; variant v's table starts n_intervals * TMH_DISPATCH_COLS * ld elements after v - 1's
 *   soc               device int64 [n_variants][ld]
 *   params            device int64 [n_variants][6 + 4 * n_rules][ld]; n_rules is the same for every variant (a
 *                     variant with fewer rules repeats one)
 *   rule_of_interval  device uint8 [n_variants][n_intervals], variant v's array n_intervals bytes after v - 1's:
 *                     two tariffs have different periods (a shared array is the special case of equal rows)
 * The table, soc and params strides are in units of ld, so column slices of wider tensors stay valid; indexing
 * within a variant is per chain index (ids[slot] under tmh_set_chain_ids).  Entries at or above n_rules and
 * interval indices past the array are clamped per variant as a lane loads them, as tmh_schedule's: no address
 * depends on an unchecked value.  work: the battery sweep's, >= tmh_battery_sweep_work_bytes(n_chains, n_steps,
 * n_variants) bytes of the largest window.  The engine runs the variants in groups of a compile-time count per
 * launch (a group of one variant is tmh_schedule's own launches on that variant's array row); the bits do not
 * depend on the grouping, windows, pipelining, batches or compaction.  fp64 engines and the engine's one site
 * only.  n_variants takes tmh_schedule's tail padding: sizeof(tmh_schedule_sweep) == sizeof(tmh_schedule). */
#define TMH_SCHEDULE_SWEEP_MAX 16
typedef struct tmh_schedule_sweep {
    tmh_intervals table;      /* sum is [n_variants][n_intervals][TMH_DISPATCH_COLS][ld] */
    int64_t* soc;             /* device [n_variants][ld] */
    void* work;               /* device scratch */
    size_t work_bytes;        /* >= tmh_battery_sweep_work_bytes(n_chains, n_steps, n_variants) of the largest window */
    const int64_t* params;    /* device [n_variants][6 + 4 * n_rules][ld] */
    const uint8_t* rule_of_interval;   /* device [n_variants][n_intervals] */
    uint32_t n_rules;         /* 1 .. TMH_SCHEDULE_RULES_MAX, the same for every variant */
    uint32_t n_variants;      /* 1 .. TMH_SCHEDULE_SWEEP_MAX */
} tmh_schedule_sweep;

/* The dispatch fleet series: the battery fleet series (TMH_BATTERY_FLEET_COLS above) behind battery dispatch or
 * scheduled dispatch -- what the whole batch draws, feeds in, curtails and stores second by second under a feed-in
 * limit, thresholds, a tariff or grid charging.  The coincidence across chains within an interval is what no
 * table holds: the sum of the chains' peaks (columns 11 and 12) is not the fleet's peak.  An output of the kind
 * beside its interval table (never instead of it), filled by the replay pass of tmh_set_dispatch or of
 * tmh_set_schedule, whichever is set.  The descriptor is tmh_series with TMH_DISPATCH_FLEET_COLS columns per row:
 * sum is device int64 [n_groups][n_steps][9], accumulated over calls (the caller zero-initialises); the ok rule
 * and the groups are the fleet series' (chain i of a call in group i / group_chains, 0: one group, else a
 * multiple of 512).  Row s of a group holds, for step step0 + s, over the group's chains that are ok at that step:
 *   [0..3] tmh_series' columns (sum of q(pv), sum of q(meter), n_ok, covered), bit for bit
 *   [4] sum of import_b     what the fleet draws from the grid (grid charging included)
 *   [5] sum of export_b     what it feeds in, after the limit
 *   [6] sum of x'           the state of charge after the second, in 2^-12 W s
 *   [7] sum of max(b, 0)    what the batteries take at the meter side
 *   [8] sum of curtailed    what the inverters throw away above the limit
 * with import_b, export_b, b, x' and curtailed exactly tmh_dispatch's per-second quantities; under a schedule
 * they are tmh_schedule's, with the rule of the second's own interval.  For every row [4] - [5] - [8] == [1] - [0]
 * + sum of b, so the fleet's net battery power follows from the row and its discharging power is [7] - sum of b
 * >= 0; columns 4-8 are >= 0; [6] <= the sum of C over the group; where every chain of the group has the same
 * limit L, [5] <= n_ok * L.  A chain that is not ok at a second adds nothing to that row, its stored energy
 * included.  With Tc = Td = 0 and L = 2^27 columns 0-7 are the battery fleet series' and column 8 is 0.
 * Bounds of the kernels' 32-lane, 32-bit partial sums: under plain dispatch b lies between 0 and d, so the battery
 * fleet series' bounds hold (max(b, 0) <= q(pv) < 2^26, import_b < 2^27), and export_b + curtailed = the surplus
 * <= max(d, 0) < 2^26.  A grid-charging rule of a schedule breaks two of them: b goes up to Pc = 2^27 -- 32 lanes
 * of exactly 2^27 are 2^32 -- and import_b up to 2^26 + 2^27.  Under a schedule these two are therefore summed
 * over 16 lanes in 32 bits (16 x 3 * 2^26 < 2^32) and the two 16-lane sums added in 33 bits; export_b and
 * curtailed stay below 2^26 (the surplus r = d - b <= d), x' < 2^40 goes as two 20-bit halves as before.  Plain
 * dispatch's replay keeps the 32-lane sums.  Integer sums: the bits do not depend on block, wave, window, batch
 * or pipelining order and equal a sequential loop over the traces; several engines may add into one buffer. */
#define TMH_DISPATCH_FLEET_COLS 9

int tmh_abi_version(void);
const char* tmh_last_error(void);
/* TMH_SERIES_FRAC_BITS and TMH_SERIES_MAX_W as the library was built with them */
int tmh_series_frac_bits(void);
double tmh_series_max_w(void);
/* Provenance: "TMHSTAMP:" + the 16-hex-digit hash of the sources and compile flags
 * this library was built from (tmhpvsim_amd/build.py build_stamp; "unstamped" for a
 * build outside it).  The Python loader refuses an in-tree library whose stamp differs
 * from its sources, so a stale binary is never tested or benchmarked. */
const char* tmh_build_stamp(void);

/* Chain state (structure of arrays, one element per chain per field). */
size_t tmh_state_bytes(uint32_t n_chains);
/* byte offsets of the TMH_STATE_NFIELDS fields (order documented in DESIGN.md) */
#define TMH_STATE_NFIELDS 24
int tmh_state_offsets(uint32_t n_chains, uint64_t* offsets);

/* Device buffers a window needs:
 *  plan    (chain-independent): clock/geometry table, boundary events, block descriptors;
 *  scratch (time-parallel path): segment records, window-end state, stats partials;
 *  workspace = plan + scratch (tmh_run builds the plan itself). */
size_t tmh_plan_bytes(uint32_t n_steps);
size_t tmh_scratch_bytes(uint32_t n_chains, uint32_t n_steps);
size_t tmh_workspace_bytes(uint32_t n_chains, uint32_t n_steps);
/* The scratch this engine's time-parallel path needs (its precision sizes the minute
 * table: fp32 engines need less than tmh_scratch_bytes, which fits any engine). */
size_t tmh_engine_scratch_bytes(const struct tmh_engine* eng, uint32_t n_chains, uint32_t n_steps);
/* The segment walk's rows (16 lanes each, four per wavefront) per chain: with
 * chains_per_row = k the walk launches ceil(n / k) rows, each row starting with one
 * chain and taking the next unstarted chain of the window's queue when its chain
 * is done.  The walk's duration is set by the longest chain either way; k > 1
 * shrinks its footprint on the CUs (for callers that run several batches' walks
 * beside other kernels).  Results do not depend on k.  0 or 1 = one chain per row
 * (default); at most 64. */
int tmh_set_walk_chains_per_row(struct tmh_engine* eng, uint32_t chains_per_row);
/* Lanes per chain in the segment walk: 16 (four chains per wavefront), 8 or 4
 * (sixteen chains per wavefront, four times the sigma entries per lane); 0 = by
 * batch size (the default: 16 up to 8,192 chains, where the walk is latency-bound,
 * else 4).  Fewer lanes per chain: fewer instructions and registers per chain-call,
 * a longer chain of work per call.  Results do not depend on it. */
int tmh_set_walk_lanes(struct tmh_engine* eng, uint32_t lanes);
/* Walk rows in the order of the chains' wind over the window, windiest first (on
 * by default): the chains of one walk wavefront then make similar numbers of
 * next_cloud calls.  Set it before a window's draws (TMH_WALK_DRAWS: they compute the
 * order and store the candidate table by it).  Results do not depend on it. */
int tmh_set_walk_order(struct tmh_engine* eng, int on);
/* A HIP stream whose kernels run on a range of compute units only (no reference
 * counterpart: a scheduling helper for callers that pipeline batches).  CU-mask
 * bits cu_first .. cu_first + cu_count - 1 of the current device; the driver
 * spreads consecutive mask bits over the XCDs, so a range is an even share of
 * every XCD.  cu_count == 0: all CUs (a plain stream).  A range of every CU runs
 * anywhere like a plain stream but, being CU-masked, on a hardware queue of its own
 * (plain streams share GPU_MAX_HW_QUEUES queues round-robin, a queue running its
 * packets in order across them): the pipelines' streams (tmhpvsim_amd.pipeline).
 * *stream receives the hipStream_t; release it with tmh_stream_destroy.  The stream
 * belongs to the calling thread's current device (hipSetDevice first).  A CU-masked
 * stream is a blocking stream (it synchronises with the legacy null stream, as
 * hipStreamCreate's default does); cu_count == 0 gives a non-blocking one. */
int tmh_stream_create_cus(uint32_t cu_first, uint32_t cu_count, void** stream);
int tmh_stream_destroy(void* stream);
/* Compaction (batches whose chains fault, e.g. the reference's markov-mode
 * AssertionError, cloud_cover_binary.py:91): run later windows on the live chains
 * only.  A launch slot then holds chain ids[slot] of a full batch of n_full chains:
 * the slot's keyed draws are that chain's (chain0 + ids[slot]), and it reads row
 * ids[slot] of the per-chain shape tables and sites and accumulates into column
 * ids[slot] of tmh_stats.chain_acc ([4][n_full]).  State, scratch and traces stay
 * per slot.  ids == NULL: slot i is chain i (the default).  Results per chain do
 * not depend on the compaction. */
int tmh_set_chain_ids(struct tmh_engine* eng, const uint32_t* ids, uint32_t n_full);
/* the ids (ids_in[slot], or the slot itself when ids_in == NULL) of the slots of
 * `state` (n_chains slots) whose status is 0, in slot order, into ids_out
 * (device, n_chains entries); their count into *n_live (device uint32). */
int tmh_live_chains(struct tmh_engine* eng, const void* state, uint32_t n_chains, const uint32_t* ids_in,
                    uint32_t* ids_out, uint32_t* n_live, void* stream);
/* move chains between two state buffers: gather (scatter = 0) dst slot i <- src
 * slot map[i], scatter (1) dst slot map[i] <- src slot i, for i < min(*count, cap)
 * (count: device uint32, e.g. tmh_live_chains' n_live). */
int tmh_state_move(struct tmh_engine* eng, const void* src, uint32_t n_src, void* dst, uint32_t n_dst,
                   const uint32_t* map, const uint32_t* count, uint32_t cap, int scatter, void* stream);
/* Tests only: segment records kept per chain (a multiple of 16; 0 = the default
 * (n_steps/135 + 16) rounded up to 16) and the overflow pool's chunks (0 = n_chains/16 + 8), for
 * every later tmh_scratch_bytes / launch in this process.  Exercises the
 * overflow path, which the default sizes reach only on the windiest days. */
int tmh_test_set_segment_capacity(uint32_t cap, uint32_t pool_chunks);

int tmh_engine_create(const tmh_params* params, const tmh_clock* clock, int device,
                      struct tmh_engine** out);
int tmh_engine_destroy(struct tmh_engine* eng);
/* Replace the engine's wall clock for later plans (a rolling DST table: the
 * shift table holds 8 changes, so open-ended runs roll it forward).  Steps keep
 * their numbering (same utc0); the new clock must describe every step still to
 * be run plus the one before the first (boundary detection compares with it).
 * tmh_init keeps using the step-0 time of the creation clock. */
int tmh_set_clock(struct tmh_engine* eng, const tmh_clock* clock);
/* the kernel path the engine resolved (TMH_PATH_SEQUENTIAL or TMH_PATH_TIME_PARALLEL) */
int tmh_engine_path(const struct tmh_engine* eng);

/* Per-chain hourly cloud-cover shape tables (a lat/lon sweep with one table per
 * site).  Replaces, for every chain, the single table of
 * tmh_params.shapes / shape_is_t that get_distributions_from_shapes_file loads
 * (cloud_cover_hourly.py:269-288) and get_cloud_cover draws from (:290-316);
 * the bin edges stay tmh_params.edges.  shapes: device [n_chains][6][4] fp64
 * (loc, scale, kappa, df per bin), is_t: device [n_chains][6] int32 or NULL
 * (then tmh_params.shape_is_t).  Row i serves the chain at index i of the
 * tmh_init / tmh_run batch (chain0 + i), so n_chains must cover the batch.
 * The buffers are read by every later launch and must outlive them; shapes ==
 * NULL restores the single table; shapes must be 16-byte aligned (the markov
 * kernel stages each workgroup's rows in LDS with 16-B loads; TMH_E_INVAL
 * otherwise).  Both cc modes and both kernel paths. */
int tmh_set_shape_tables(struct tmh_engine* eng, const double* shapes, const int32_t* is_t,
                         uint32_t n_chains);

/* Per-chain PV sites (the lat/lon sweep of SURVEY C5; the reference builds one
 * PVModel per site, pvmodel.py:19-30).  sites: device [n_chains][8] fp64 rows in
 * tmh_params.site order; columns 0-5 (latitude, longitude, altitude, tilt,
 * surface azimuth, albedo) are per chain, temp_air and wind stay tmh_params'
 * (pvmodel.py:69-70 fixes them).  linke: device [n_chains][12] monthly Linke
 * turbidity or NULL (tmh_params.linke).  The clock, the boundary schedule and
 * the sun's place stay in the shared plan; solar position, clear-sky GHI,
 * DISC, POA and the SAPM factors are then evaluated per chain-second.  Row i
 * serves the chain at index i of the batch; buffers must outlive the
 * launches; sites == NULL restores the engine's single site. */
int tmh_set_sites(struct tmh_engine* eng, const double* sites, const double* linke, uint32_t n_chains);

/* Fleet series (tmh_series above): every later expansion of this engine adds its
 * window's rows to series->sum; NULL switches it off.  A setter like the two above;
 * the struct is copied, the buffer must outlive the launches.  The series is final
 * after the TMH_EXPAND_COMMIT half (it carries the fixup's corrections), as the
 * statistics are.  With a series set, a step / expansion call is refused
 * (TMH_E_INVAL, before any launch) when: a trace pointer is non-NULL (a caller with
 * traces can sum them); the engine runs the sequential path or injected uniforms;
 * chain ids are set (compaction: a tile would mix groups); the window is not inside
 * [step0, step0 + n_steps); n_groups * group_chains < n_chains; group_chains is not
 * 0 or a multiple of 512 (with 0, n_groups must be 1); inverter Paco or |Pnt| is not
 * below TMH_SERIES_MAX_W.  Per-chain statistics and the histogram are accumulated
 * beside the series when tmh_stats gives them. */
int tmh_set_series(struct tmh_engine* eng, const tmh_series* series);
/* Interval metering (tmh_intervals above): every later expansion of this engine adds its
 * window to iv->sum; NULL switches it off.  A setter like tmh_set_series; the struct is
 * copied, the buffer must outlive the launches; the table is final after the
 * TMH_EXPAND_COMMIT half.  Refused here: a NULL or misaligned (8 bytes) sum, n_steps,
 * ld or interval_s of 0.  With intervals set, a step / expansion call (and a walk of
 * that window) is refused (TMH_E_INVAL, before any launch) when: a trace pointer is
 * non-NULL; a fleet series is set too; the engine runs the sequential path or injected
 * uniforms; the window is not inside [step0, step0 + n_steps); ld is smaller than the
 * chains it must hold (n_chains, under tmh_set_chain_ids n_full); inverter Paco or |Pnt|
 * is not below TMH_SERIES_MAX_W.  Compacted windows are accepted.  Per-chain statistics
 * and the histogram are accumulated beside the intervals when tmh_stats gives them. */
int tmh_set_intervals(struct tmh_engine* eng, const tmh_intervals* iv);
/* Import / export registers (tmh_registers above): every later expansion of this engine
 * adds its window to rg->sum; NULL switches them off.  A setter like tmh_set_intervals,
 * with the same refusals here (a NULL or misaligned sum, n_steps, ld or interval_s of 0)
 * and at a step / expansion call or a walk of that window (TMH_E_INVAL, before any
 * launch): a trace pointer; a fleet series or interval metering set too (the registers
 * table holds the intervals' columns); the sequential path or injected uniforms; a window
 * outside [step0, step0 + n_steps); ld too small; inverter Paco or |Pnt| not below
 * TMH_SERIES_MAX_W.  Compacted windows are accepted.  Statistics and the histogram are
 * accumulated beside the registers when tmh_stats gives them.  The table is final after
 * the TMH_EXPAND_COMMIT half. */
int tmh_set_registers(struct tmh_engine* eng, const tmh_registers* rg);
/* Demand registers (tmh_demand above): every later expansion of this engine adds its window
 * to dm->sum (columns 0-5 by addition, 6 and 7 by maximum); NULL switches them off.  A setter
 * like tmh_set_registers, with the same refusals here and at a step / expansion call or a
 * walk of that window (TMH_E_INVAL, before any launch; the messages name "demand"), and also:
 * a fleet series, interval metering or the import / export registers set too, in either
 * order (the demand table holds their columns).  Compacted windows are accepted.  Statistics
 * and the histogram are accumulated beside the table when tmh_stats gives them.  The table
 * is final after the TMH_EXPAND_COMMIT half. */
int tmh_set_demand(struct tmh_engine* eng, const tmh_demand* dm);
/* Battery storage (tmh_storage above): every later expansion of this engine advances
 * st->soc over its window and adds the window to st->table.sum; NULL switches it off.  The
 * expansion then runs three launches on its stream (TMH_EXPAND_KERNEL half): a map pass
 * (each chain's 128-step blocks as composed SoC maps), a scan (each block's starting SoC) and
 * the replay pass that writes the table; windows must run in order.  Refused here
 * (TMH_E_INVAL, the messages name "storage"): tmh_set_intervals' bad-struct cases; a NULL or
 * misaligned (8 bytes) soc or work; capacity outside [0, 2^40), p_charge or p_discharge
 * outside [0, 2^27]; interval_s > 2^23 - 1; an fp32 engine.  Refused at a step / expansion
 * call or a walk of that window, before any launch: everything tmh_set_registers refuses; any
 * other interval table or a fleet series set too, in either order; work_bytes below
 * tmh_storage_work_bytes of this window.  Compacted windows are accepted.  Statistics and the
 * histogram are accumulated beside the table when tmh_stats gives them.  tmh_scratch_bytes
 * and tmh_engine_scratch_bytes do not change: the caller owns every buffer. */
size_t tmh_storage_work_bytes(uint32_t n_chains, uint32_t n_steps);
int tmh_set_storage(struct tmh_engine* eng, const tmh_storage* st);
/* The battery kind (tmh_battery above): as tmh_set_storage, with the parameters in memory.
 * Every later expansion clamps bt->soc into [0, C], advances it over its window and adds
 * the window to bt->table.sum, in tmh_set_storage's three launches (timed by the same
 * TMH_K_STORAGE_* slots); NULL switches it off.  Refused here (TMH_E_INVAL, the messages name
 * "battery"): everything tmh_set_storage refuses of the table, soc, work and the engine; a
 * NULL or misaligned (8 bytes) params.  Refused at a step / expansion call or a walk of that
 * window, before any launch: everything tmh_set_storage's step refuses; battery storage
 * (tmh_set_storage) set too, in either order.  The parameters' values are not read on the
 * host: the kernels clamp them. */
int tmh_set_battery(struct tmh_engine* eng, const tmh_battery* bt);
/* The battery fleet series (TMH_BATTERY_FLEET_COLS above): every later expansion of this engine with the
 * battery kind set adds its window's rows to fleet->sum, in the kind's replay pass, beside the kind's
 * table; NULL switches it off.  The descriptor is tmh_series with eight columns per row; a setter like
 * tmh_set_series: the struct is copied, the buffer must outlive the launches, the rows are final after
 * the TMH_EXPAND_KERNEL half.  Refused here (TMH_E_INVAL, the messages name "battery fleet"):
 * tmh_set_series' bad-struct cases (no buffer, a misaligned one, n_steps or n_groups 0, group_chains not
 * 0 with one group or a multiple of 512); an fp32 engine.  Refused at a step / expansion call or a walk
 * of that window, before any launch and naming "battery fleet": no battery kind set (tmh_set_battery);
 * battery storage set (tmh_set_storage, the lossless kind: use the battery kind with efficiencies 1);
 * chain ids set (compaction: a tile would mix groups, as for the series); a window not inside [step0,
 * step0 + n_steps); n_groups * group_chains < n_chains.  Everything tmh_set_battery's step refuses stays
 * refused in its words, tmh_set_series beside the kind included.  Statistics and the histogram are
 * accumulated beside both when tmh_stats gives them. */
int tmh_set_battery_fleet(struct tmh_engine* eng, const tmh_series* fleet);
/* The battery sweep (tmh_battery_sweep above): every later expansion of this engine advances
 * sw->soc and adds its window to sw->table.sum for each of the n_variants batteries of every chain;
 * NULL switches it off.  The variants run in groups, each group in the battery kind's three
 * launches; TMH_K_STORAGE_MAP, TMH_K_STORAGE_SCAN and TMH_K_STORAGE_REPLAY sum this kind's launches
 * of a window and TMH_K_EXPAND spans all of them.  Statistics and the histogram, when tmh_stats
 * gives them, are accumulated by exactly one replay launch per window.  Refused here (TMH_E_INVAL,
 * the messages name "battery sweep"): tmh_set_battery's bad-struct cases; n_variants 0 or above
 * TMH_BATTERY_SWEEP_MAX; a NULL or misaligned (8 bytes) params, soc or work; work_bytes below
 * tmh_battery_sweep_work_bytes(1, 1, n_variants); an fp32 engine.  Refused at a step / expansion
 * call or a walk of that window, before any launch: everything tmh_set_battery's step refuses (the
 * work buffer against tmh_battery_sweep_work_bytes of the window); any other table kind set too, in
 * either order, battery storage and the battery kind included; tmh_set_series or
 * tmh_set_battery_fleet set; per-chain sites (tmh_set_sites). */
size_t tmh_battery_sweep_work_bytes(uint32_t n_chains, uint32_t n_steps, uint32_t n_variants);
int tmh_set_battery_sweep(struct tmh_engine* eng, const tmh_battery_sweep* sw);
/* Battery dispatch (tmh_dispatch above): as tmh_set_battery, with nine parameter rows and thirteen columns.
 * Every later expansion clamps dp->soc into [0, C], advances it over its window and adds the window to
 * dp->table.sum in the battery kind's three launches (the same TMH_K_STORAGE_* slots time them); NULL
 * switches it off.  Refused here (TMH_E_INVAL, the messages name "dispatch"): everything tmh_set_battery
 * refuses.  Refused at a step / expansion call or a walk of that window, before any launch: everything
 * tmh_set_battery's step refuses; any other table kind set too, in either order (battery storage, the
 * battery kind and the battery sweep included); a fleet series set too; tmh_set_battery_fleet set too.  The
 * parameters' values are not read on the host: the kernels clamp them. */
int tmh_set_dispatch(struct tmh_engine* eng, const tmh_dispatch* dp);
/* The dispatch sweep (tmh_dispatch_sweep above): every later expansion of this engine advances sw->soc and
 * adds its window to sw->table.sum for each of the n_variants rule sets of every chain; NULL switches it off.
 * The variants run in groups, each group in the kind's three launches; TMH_K_STORAGE_MAP, TMH_K_STORAGE_SCAN
 * and TMH_K_STORAGE_REPLAY sum this kind's launches of a window and TMH_K_EXPAND spans all of them.  Statistics
 * and the histogram, when tmh_stats gives them, are accumulated by exactly one replay launch per window.
 * Refused here (TMH_E_INVAL, the messages name "dispatch sweep"): tmh_set_dispatch's bad-struct cases;
 * n_variants 0 or above TMH_DISPATCH_SWEEP_MAX; a NULL or misaligned (8 bytes) params, soc or work; work_bytes
 * below tmh_battery_sweep_work_bytes(1, 1, n_variants); an fp32 engine.  Refused at a step / expansion call or
 * a walk of that window, before any launch: everything tmh_set_dispatch's step refuses (the work buffer against
 * tmh_battery_sweep_work_bytes of the window); any other table kind set too, in either order, the battery
 * sweep and battery dispatch included; tmh_set_series or tmh_set_battery_fleet set; per-chain sites
 * (tmh_set_sites). */
int tmh_set_dispatch_sweep(struct tmh_engine* eng, const tmh_dispatch_sweep* sw);
/* Scheduled dispatch (tmh_schedule above): as tmh_set_dispatch, with 6 + 4 * n_rules parameter rows and the rule
 * array.  Every later expansion clamps sc->soc into [0, C], advances it over its window and adds the window to
 * sc->table.sum in the battery kind's three launches (the same TMH_K_STORAGE_* slots time them); NULL switches
 * it off.  Refused here (TMH_E_INVAL, the messages name "schedule"): everything tmh_set_dispatch refuses;
 * n_rules 0 or above TMH_SCHEDULE_RULES_MAX; a NULL rule_of_interval; work_bytes below
 * tmh_storage_work_bytes(1, 1).  Refused at a step / expansion call or a walk of that window, before any launch:
 * everything tmh_set_dispatch's step refuses (traces, the work buffer against the window, ...); any other table
 * kind set too, in either order; tmh_set_series or tmh_set_battery_fleet set; per-chain sites (tmh_set_sites).
 * The parameters' and the array's values are not read on the host: the kernels clamp them. */
int tmh_set_schedule(struct tmh_engine* eng, const tmh_schedule* sc);
/* The schedule sweep (tmh_schedule_sweep above): every later expansion of this engine advances sw->soc and adds
 * its window to sw->table.sum for each of the n_variants (battery, rules, array) variants of every chain; NULL
 * switches it off.  The variants run in groups, each group in the kind's three launches; the TMH_K_STORAGE_* slots
 * sum this kind's launches of a window and TMH_K_EXPAND spans all of them.  Statistics and the histogram, when
 * tmh_stats gives them, are accumulated by exactly one replay launch per window.  tmh_engine_last_expand reports
 * TMH_OUT_SCHEDULE_SWEEP | TMH_OUT_FP64.  Refused here (TMH_E_INVAL, the messages name "schedule sweep"):
 * tmh_set_schedule's bad-struct cases; n_variants 0 or above TMH_SCHEDULE_SWEEP_MAX; n_rules 0 or above
 * TMH_SCHEDULE_RULES_MAX; a NULL or misaligned (8 bytes) params, soc or work; a NULL rule_of_interval; work_bytes
 * below tmh_battery_sweep_work_bytes(1, 1, n_variants); an fp32 engine.  Refused at a step / expansion call or a
 * walk of that window, before any launch: everything tmh_set_schedule's step refuses (traces; the work buffer
 * against tmh_battery_sweep_work_bytes of the window); any other table kind set too, in either order;
 * tmh_set_series, tmh_set_battery_fleet or tmh_set_dispatch_fleet set; per-chain sites (tmh_set_sites).  The
 * parameters' and the arrays' values are not read on the host: the kernels clamp them. */
int tmh_set_schedule_sweep(struct tmh_engine* eng, const tmh_schedule_sweep* sw);
/* The dispatch fleet series (TMH_DISPATCH_FLEET_COLS above): every later expansion of this engine with battery
 * dispatch or the schedule set adds its window's rows to fleet->sum, in the kind's replay pass, beside the kind's
 * table; NULL switches it off.  The kind's table and soc are exactly what they are without the series.  A setter
 * like tmh_set_battery_fleet: the struct is copied, the buffer must outlive the launches, the rows are final after
 * the TMH_EXPAND_KERNEL half.  Refused here (TMH_E_INVAL, the messages name "dispatch fleet series"):
 * tmh_set_battery_fleet's bad-struct cases; an fp32 engine.  Refused at a step / expansion call or a walk of that
 * window, before any launch and naming "dispatch fleet series": neither tmh_set_dispatch nor tmh_set_schedule set;
 * any other table kind set; tmh_set_series or tmh_set_battery_fleet set too; chain ids set (compaction); per-chain
 * sites (tmh_set_sites: one feeder is one site); a window not inside [step0, step0 + n_steps); n_groups *
 * group_chains < n_chains.  Everything the kind's step refuses without the series stays refused in its words
 * (tmh_set_battery_fleet beside dispatch or the schedule included).  Statistics and the histogram are accumulated
 * beside both when tmh_stats gives them. */
int tmh_set_dispatch_fleet(struct tmh_engine* eng, const tmh_series* fleet);
/* Tests only: the fp32 guard-band records (chain, block) the last expansion on
 * `scratch` (laid out for n_chains x n_steps) appended; a synchronous copy from the
 * device (the caller has synchronised the expansion's stream).  Negative: TMH_E_*. */
int64_t tmh_test_guard_records(const struct tmh_engine* eng, const void* scratch, uint32_t n_chains,
                               uint32_t n_steps);

/* ClearskyindexModel.__init__ for chains [chain0, chain0 + n_chains): the 14+
 * constructor draws and CloudCoverBinary's first cloud.  `inj` may be NULL
 * (keyed mode). */
int tmh_init(struct tmh_engine* eng, void* state, uint64_t chain0, uint32_t n_chains,
             const tmh_ustream* inj, void* stream);

/* Advance the chains over steps [step0, step0 + n_steps): per second the
 * hourly/daily/minute resampling, the cloud-cover binary, the clear-sky index,
 * the PV chain, the meter draw and the residual, fused.  Writes traces and/or
 * accumulates statistics.  = tmh_plan + tmh_step on `workspace`
 * (tmh_workspace_bytes(n_chains, n_steps) bytes). */
int tmh_run(struct tmh_engine* eng, void* state, uint64_t chain0, uint32_t n_chains,
            int64_t step0, uint32_t n_steps, const tmh_ustream* inj, const tmh_trace* trace,
            const tmh_stats* stats, void* workspace, size_t workspace_bytes, void* stream);

/* Build the chain-independent plan of the window [step0, step0 + n_steps) into
 * `plan` (tmh_plan_bytes(n_steps) bytes).  The first TMH_GEOM_FIELDS * n_steps
 * doubles are the clock/geometry table (row layout in DESIGN.md).  One plan
 * serves every chain batch of the same site and window.  A plan is read-only
 * from here on: nothing may write to it while a walk or an expansion that was
 * given it is still running (the expansion reads its rows as constant memory);
 * reuse the buffer for another window only after those have finished. */
int tmh_plan(struct tmh_engine* eng, int64_t step0, uint32_t n_steps, void* plan, void* stream);

/* tmh_run on a plan built by tmh_plan(step0, n_steps) for this engine. */
int tmh_step(struct tmh_engine* eng, void* state, uint64_t chain0, uint32_t n_chains,
             int64_t step0, uint32_t n_steps, const tmh_ustream* inj, const tmh_trace* trace,
             const tmh_stats* stats, const void* plan, void* scratch, size_t scratch_bytes,
             void* stream);

/* tmh_step in its two halves, for callers that overlap independent batches
 * (bench.py: the latency-bound segment walks of the next batches run beside
 * this batch's expansion).  tmh_walk: boundary draws, candidate cloud lengths
 * and the P1 segment walk into `scratch`; tmh_expand: the P2 expansion
 * (traces / statistics) and the state commit from that scratch.  Call them in
 * this order on the same plan, scratch and state (the same stream, or with the
 * caller ordering them); tmh_step == tmh_walk + tmh_expand.  On the sequential
 * path tmh_walk does nothing and tmh_expand runs the whole step. */
int tmh_walk(struct tmh_engine* eng, void* state, uint64_t chain0, uint32_t n_chains, int64_t step0,
             uint32_t n_steps, const void* plan, void* scratch, size_t scratch_bytes, void* stream);
int tmh_expand(struct tmh_engine* eng, void* state, uint64_t chain0, uint32_t n_chains, int64_t step0,
               uint32_t n_steps, const tmh_ustream* inj, const tmh_trace* trace, const tmh_stats* stats,
               const void* plan, void* scratch, size_t scratch_bytes, void* stream);

/* The walk in parts and across windows (time-parallel path).
 * parts: TMH_WALK_DRAWS = boundary draws, markov hourly cover, candidate cloud
 * lengths and the window's minute draws (many small workgroups); TMH_WALK_SEGMENTS = the P1 segment walk (one
 * wave per SIMD, long-lived).  Small grids issued beside a running expansion
 * wait for CU slots, so a pipelining caller puts the draws on the expansion's
 * stream and only the segment walk on a second, high-priority stream.
 * prev_scratch (nullable): the scratch (laid out for prev_n_steps) of the previous
 * window of these chains; the window-start status, cloud-cover and wind pairs then
 * come from that window's walk instead of the state, so this walk may run while
 * the previous window's expansion and commit are in flight.  Order: draws(w+1)
 * after segments(w); segments(w+1) after draws(w+1); expand(w+1) after
 * segments(w+1) and expand(w); any part of w+2 after expand(w), the last reader
 * of the buffers w+2 reuses (BatchedSim.run, bench.py).  Same bits as tmh_step
 * window by window. */
#define TMH_WALK_DRAWS 1
#define TMH_WALK_SEGMENTS 2
int tmh_walk_part(struct tmh_engine* eng, void* state, uint64_t chain0, uint32_t n_chains, int64_t step0,
                  uint32_t n_steps, const void* plan, void* scratch, size_t scratch_bytes,
                  const void* prev_scratch, uint32_t prev_n_steps, int parts, void* stream);

/* tmh_expand in its two halves, for callers that overlap independent batches
 * (bench.py): TMH_EXPAND_KERNEL = the P2 expansion (traces / statistics);
 * TMH_EXPAND_COMMIT = the fp32 guard-band recomputation (fixup) and the state /
 * statistics commit.  The commit half is latency-bound (a few waves); on a second
 * stream, after an event recorded behind the kernel half, it runs beside the next
 * batch's expansion.  Order: KERNEL then COMMIT on the same buffers; the traces and
 * statistics are final after COMMIT.  tmh_expand == KERNEL | COMMIT.  The window's
 * minute draws are part of TMH_WALK_DRAWS (one launch with the candidate lengths,
 * built with the construction, off the expansion's stream); TMH_EXPAND_MINUTES and
 * TMH_EXPAND_NO_MINUTES (round 3's split of them) are accepted and do nothing. */
#define TMH_EXPAND_KERNEL 1
#define TMH_EXPAND_COMMIT 2
#define TMH_EXPAND_MINUTES 4
#define TMH_EXPAND_NO_MINUTES 8
int tmh_expand_part(struct tmh_engine* eng, void* state, uint64_t chain0, uint32_t n_chains, int64_t step0,
                    uint32_t n_steps, const tmh_ustream* inj, const tmh_trace* trace, const tmh_stats* stats,
                    const void* plan, void* scratch, size_t scratch_bytes, int parts, void* stream);

/* Kernel timing (measurement only).  While enabled, tmh_step records HIP
 * events, on the stream each kernel runs on, around the kernels of the
 * time-parallel path; tmh_profile_read waits for them and returns the summed
 * milliseconds and launch count of one kernel since the last read, then resets
 * it.  kernel: TMH_K_EXPAND (P2 trace/stats expansion), TMH_K_SEGMENTS (P1
 * segment walk), TMH_K_CANDIDATES (P1's candidate table), TMH_K_STEP (the
 * whole tmh_step); with battery storage or the battery kind set, TMH_K_EXPAND spans the kind's three launches
 * and TMH_K_STORAGE_MAP, TMH_K_STORAGE_SCAN and TMH_K_STORAGE_REPLAY time each of them (the battery sweep and the dispatch sweep:
 * each slot sums that launch over the window's groups of variants, several launches per read). */
enum { TMH_K_EXPAND = 0, TMH_K_SEGMENTS = 1, TMH_K_CANDIDATES = 2, TMH_K_STEP = 3, TMH_K_STORAGE_MAP = 4,
       TMH_K_STORAGE_SCAN = 5, TMH_K_STORAGE_REPLAY = 6, TMH_K_COUNT = 7 };
int tmh_profile_enable(struct tmh_engine* eng, int on);
int tmh_profile_read(struct tmh_engine* eng, int kernel, double* total_ms, int* launches);

/* The expansion variant the engine's last tmh_step / tmh_expand(_part) launched
 * (tests and measurement: which kernel instantiation produced a line or a trace):
 * TMH_OUT_ANY (any trace fields and/or statistics), TMH_OUT_TRACE3 (exactly pv,
 * meter, residual, no statistics: the trace-mode hot path), TMH_OUT_STATS
 * (statistics only), TMH_OUT_SERIES (a fleet series, with or without statistics),
 * TMH_OUT_INTERVALS (interval metering, with or without statistics),
 * TMH_OUT_REGISTERS (import / export registers, with or without statistics),
 * TMH_OUT_DEMAND (demand registers, with or without statistics), TMH_OUT_STORAGE (battery
 * storage: the replay pass, the last of the kind's three launches, with or without statistics),
 * TMH_OUT_BATTERY (the battery kind, likewise), TMH_OUT_BATTERY_FLEET (the battery kind with its fleet
 * series: the replay pass that fills both), TMH_OUT_BATTERY_SWEEP (the battery sweep),
 * TMH_OUT_DISPATCH (battery dispatch: its replay pass, with or without statistics),
 * TMH_OUT_DISPATCH_SWEEP (the dispatch sweep), TMH_OUT_SCHEDULE (scheduled dispatch: its replay pass),
 * TMH_OUT_DISPATCH_FLEET and TMH_OUT_SCHEDULE_FLEET (battery dispatch / the schedule with the dispatch fleet
 * series: the replay pass that fills both), TMH_OUT_SCHEDULE_SWEEP (the schedule sweep: codes 0-15 are used
 * up, so it is the first value above the two flags and never a combination of them), plus
 * TMH_OUT_SITES with per-chain sites and TMH_OUT_FP64 in fp64; -1 before the first expansion (and on the sequential path, whose one
 * kernel serves every output). */
#define TMH_OUT_ANY 0
#define TMH_OUT_TRACE3 1
#define TMH_OUT_STATS 2
#define TMH_OUT_SERIES 3
#define TMH_OUT_INTERVALS 4
#define TMH_OUT_REGISTERS 5
#define TMH_OUT_DEMAND 6
#define TMH_OUT_STORAGE 7
#define TMH_OUT_BATTERY 8
#define TMH_OUT_BATTERY_FLEET 9
#define TMH_OUT_BATTERY_SWEEP 10
#define TMH_OUT_DISPATCH 11
#define TMH_OUT_DISPATCH_SWEEP 12
#define TMH_OUT_SCHEDULE 13
#define TMH_OUT_DISPATCH_FLEET 14
#define TMH_OUT_SCHEDULE_FLEET 15
#define TMH_OUT_SITES 16
#define TMH_OUT_FP64 32
#define TMH_OUT_SCHEDULE_SWEEP 64
int tmh_engine_last_expand(const struct tmh_engine* eng);

/* Device math probes for parity tests: out[i] = f(a, x[i]) with
 * f = 0 ndtri, 1 gammaincinv, 2 stdtrit, 3 al_ppf, 4 ndtri (fp32 path),
 * 8 ocml's ndtri (the fp64 noise quantile's tails), 9 / 10 the fp32 PV chain's
 * v_med3_f32 clamps med3(x, 0, a) / med3(x, -inf, a), and the fp64 PV chain's
 * table functions: 11 the noise quantile of the 32-bit word x[i], 12 log, 13 exp;
 * 17 the segment walk's cloud-length power pow(x[i], a) as the walk calls it. */
int tmh_probe(int fn, double a, const double* x, double* out, uint32_t n, void* stream);

/* The per-second PV chain on given geometry rows, for parity tests (a test hook like tmh_probe; additive,
 * TMH_ABI_VERSION stays 1).  rows: [n][TMH_GEOM_FIELDS] fp64 in the layout of the plan's table (real rows, or
 * rows with fields planted at a discontinuity of the chain); csi: [n] fp64; out: [n][3] fp64 --
 *   out[i][0]  the fp64 chain on row i with the engine's folded constants,
 *   out[i][1]  the fp32 chain on the fp32 row the single-site table holds for row i (the same conversion),
 *   out[i][2]  1 when that fp32 second lies in a guard band (the kernels recompute it in fp64), else 0.
 * The night flag is not consulted: the chain runs on every row given.  All device pointers. */
int tmh_probe_pv(struct tmh_engine* eng, const double* rows, const double* csi, double* out, uint32_t n,
                 void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TMHPVSIM_H */
