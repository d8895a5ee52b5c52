/* alifmm.h — C-ABI of libalifmm.so, the MI355X (gfx950) ALI-FMM travel-time-field solver and
 * ray tracer.  Drop-in boundary for the hot path of the reference module Anis_TTF_rays.py
 * (WiPi-UoS/ALI-FMM-and-ray-tracing); each entry point names the reference interface it replaces.
 *
 * Conventions: every function returns 0 on success and a negative code on failure, with the
 * message available from alifmm_last_error(ctx).  Host buffers are caller-owned, C-contiguous,
 * row-major [iz][ix] (the reference's numpy layout).  Device memory is library-owned.  Calls are
 * synchronous (they return after their device work and any device->host copy completed).
 * One context drives one GPU; a context is not re-entrant (one host thread per context).
 */
#ifndef ALIFMM_H
#define ALIFMM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct alifmm_ctx alifmm_ctx;

enum {
  ALIFMM_OK = 0,
  ALIFMM_E_HIP = -1,      /* HIP runtime error (device missing, out of memory, launch failure) */
  ALIFMM_E_ARG = -2,      /* invalid argument (shape, source outside the grid, no model) */
  ALIFMM_E_CAPACITY = -3, /* a device work list overflowed even after the automatic retry */
  ALIFMM_E_KERNEL = -4    /* a kernel reported an internal error (init heap overflow, ...) */
};

const char* alifmm_version(void);
int alifmm_device_count(int* n);

/* Create a context on HIP device `device` (index into the visible devices). */
int alifmm_ctx_create(int device, alifmm_ctx** out);
int alifmm_ctx_destroy(alifmm_ctx* ctx);
const char* alifmm_last_error(alifmm_ctx* ctx);

/* Upload the model (replaces the model arrays handed to travel()/travel_finer_grid()/find_ray():
 * Anis_TTF_rays.py:1464, :2121, :3105; stored by ALI_FMM.__init__ :3793-3862).
 *   veln     (nnz, nnx) float64  orientation [deg]
 *   velpn    (nnz, nnx) int64    material column; 0 selects the per-cell stiffness
 *   vel_map  (nnz, nnx) float64  velocity scale
 *   stif_den (nnz, nnx, 5) int64 c22, c23, c33, c44 [MPa], density [kg/m^3]; NULL = None
 *   group_tab, phase_tab (361, ncol) float64  velocity tables (ALI_FMM.velocity_dat / phase_vel)
 *   dnx, dnz grid spacing [m]; gox, goz origin [m]
 * ncol must be below 32768 (the init kernels pack velpn and ncol into one int): ALIFMM_E_ARG.    */
int alifmm_set_model(alifmm_ctx* ctx, int nnz, int nnx, const double* veln, const int64_t* velpn,
                     const double* vel_map, const int64_t* stif_den, const double* group_tab,
                     const double* phase_tab, int ncol, double dnx, double dnz, double gox, double goz);

/* Tuning: "members" (workgroups per source of the band kernel: 0 = as many as the device holds
 * for the batch, else 1 .. 16, lowered to the number of column stripes on a narrow grid; results
 * are bit-identical for every value), "stripe_log"
 * (column-stripe width log2 of the band kernel's ownership, 0 = automatic), "xcd_local" (1, the
 * default: once every member of a source reports the same XCD, the cross-member exchange stores
 * plainly into that XCD's L2; 0: always write-through (sc1) stores, the path members on different
 * XCDs take; bit-identical), "prof" (1: record the
 * band profile, alifmm_band_profile), "cdelta" (band width in units of dnx/vmax; unset, the
 * library chooses it per model: 0.5, narrowed down to 0.2 where the materials change from cell to
 * cell — fraction of neighbour pairs with different materials ("mat_jump", / subgrid) from 0.3 to
 * 0.6; get_option reads the subgrid-1 value),
 * "r0" (near-source band schedule radius in cells, default 40), "exact_r" (radius in cells of the
 * exact heap-ordered main-loop prefix, 0..48, default 20), "batch" (sources per launch, default
 * 256), "exact_lds" (subgrid > 1: 1 = the exact walk with its state in LDS, fmm_exact_lds.hip,
 * where the stage grids fit — subgrid <= 9; 0 = the HBM walk, fmm_exact.hip; bit-identical),
 * "coop" (band launch: 1 = cooperative, 0 = plain after a residency check), "cdelta_far" /
 * "r_far" (band width beyond Tmin = r_far * dnx / vmax, ramped in over r_far .. 2 r_far; default
 * 1.4 x the band width in force from 768 cells (0.7 at 0.5); a value set is never narrower than
 * the band width in force; cdelta_far 0 = one width everywhere), "far_sg" (the largest subgrid the
 * far band applies to, default 1), "stream_out" (subgrid-1 travels
 * with a host destination stream the fields out of the band kernel, alifmm_travel_into; default 1),
 * "init_reuse" (subgrid 1; default 1: a source whose initialisation would read exactly what the
 * initialisation that last filled its slot read — the same node, spacings, exact_r, stop time,
 * grid shape and velocity tables, and bit-identical materials in every cell within
 * max(exact_r + 6, 16) cells of it — is not initialised again: its hand-over to the band kernel is
 * still in device memory.  Decided on the device by comparing those inputs byte for byte, so the
 * fields never change; 0: every source is initialised on every call). */
int alifmm_set_option(alifmm_ctx* ctx, const char* name, double value);
/* Read an option, or "last_k" (workgroups per source of the last band launch), "n_cu"
 * (compute units of the device), "cdelta" / "cdelta_far" (the widths in force for the resident
 * model), "mat_jump" (the model's fraction of 4-neighbour cell pairs whose materials differ),
 * "vmax" (the model's fastest speed [m/s]: the exact prefix
 * covers T <= exact_r * dnx / vmax), "stream_tail_ms" and "stream_fallback" (last travel with a host
 * destination: ms from the band kernel's end to the last streamed tile copied; fields copied after
 * the launch instead of streamed), "exact_redo" (last travel, subgrid > 1: sources the LDS exact
 * walk handed to the HBM walk), "init_reused" (last travel, subgrid 1: sources whose
 * initialisation was skipped under "init_reuse"; read-only), "fill_wait_ms" (last travel: ms its
 * band launches waited, after the source initialisation, for the working fields' fills on the
 * second stream — what a skipped initialisation no longer hides), "nmat" (distinct material records of the model; 0 when there are
 * more than the id table holds), "ray_lanes" (lanes per ray of the last find_rays launch: 9, 16, 32
 * or 64), "seed_ms", "seed_nodes" and "seed_close" (last alifmm_travel_seeded: ms of its seed pass,
 * its seeds and the close cells handed over with them). */
int alifmm_get_option(alifmm_ctx* ctx, const char* name, double* value);

/* Shape of a travel-time field for subgrid size sg: (sg*(nnz-1)+1, sg*(nnx-1)+1). */
int alifmm_field_shape(alifmm_ctx* ctx, int subgrid, int* fnz, int* fnx);

/* First-arrival travel-time fields for nsrc sources (scx, scz in metres).
 * Replaces travel() :1463-2117 (subgrid == 1) and travel_finer_grid() :2120-2832 (subgrid > 1,
 * odd; the result is already divided by subgrid as at :2832).  The fields stay resident on the
 * device in slots first_slot .. first_slot+nsrc-1 (for alifmm_find_rays); if out != NULL they are
 * also copied to out (nsrc x fnz x fnx float64).  Field semantics: SURVEY/DESIGN parity contract. */
int alifmm_travel(alifmm_ctx* ctx, int subgrid, int nsrc, const double* scx, const double* scz,
                  int first_slot, double* out);

/* alifmm_travel() with a caller-owned destination per source: field i goes to dst[i] (pageable
 * host memory, fnz x fnx float64 each; e.g. rows of the (nsrc, fnz, fnx) stack of
 * ALI_FMM.update() :3870-3936, which need not be consecutive).  Subgrid 1: the band kernel
 * streams every tile of a field (one member's stripe, a few thousand cells) to a ring of coherent
 * pinned slots as soon as all its cells are final, and the context's copy threads move it on to
 * dst[i] while the band runs (option "stream_out", default 1; "stream_tail_ms" = the time from the
 * kernel's end to the last tile copied).  Otherwise (and for a field a tile of which did not
 * arrive) the fields are copied after the launch, as alifmm_copy_fields() kind 0.  The fields also
 * stay resident in slots first_slot .. first_slot+nsrc-1. */
int alifmm_travel_into(alifmm_ctx* ctx, int subgrid, int nsrc, const double* scx, const double* scz,
                       int first_slot, double* const* dst);

/* Travel-time fields from a set of seed nodes with given times instead of a point source: the
 * reflected leg of a half-skip path (the incident field's values on the reflector, frozen, and the
 * march restarted from them: multi-stage FMM) and fronts that are no points (a plane wave: the array
 * line seeded with the steering delays).  The reference has no counterpart.  Subgrid 1 only.
 *   nfield             fields of the call; they land in slots first_slot .. first_slot + nfield - 1
 *                      and stay resident, as with alifmm_travel
 *   seed_iz, seed_ix   int32 [nseed] the seed nodes, shared by all fields
 *   seed_t             float64 [nfield][nseed] host times, or NULL
 *   from_slot          int32 [nfield] resident subgrid-1 fields to read the times from, or NULL:
 *                      seed k of field i has the time field(from_slot[i])[seed_iz[k]][seed_ix[k]], read
 *                      on the device with no host round trip (64 incident fields in, 64 reflected
 *                      fields out, one call)
 *   out (nullable)     float64 [nfield][nnz][nnx], copied after the launches
 * Exactly one of seed_t and from_slot is given.
 * 1. Seeds.  The seeds are known with their times exactly as given and are never re-evaluated
 *    (Dirichlet values).  Any node set: one node, a line, several layers, scattered nodes.
 * 2. Step -1.  Every in-grid 4-neighbour of a seed that is no seed becomes close.  Its value is one
 *    band step's evaluate-and-commit with all seeds as the accepted set: update(), and where that
 *    returns -1 the fouds18_A() fallback, Jacobi-style against the seeds-only state (every other
 *    node far, ttn 0), with the device functions and the material path of the band kernel's
 *    evaluate phase.
 * 3. Hand-over and band run.  The hand-over lists the seeds in list order as known, then the close
 *    cells in ascending cell index iz * nnx + ix: its order is a function of the node list alone.
 *    The band kernel then runs unchanged with the context's band options in force.  Its schedule (the
 *    "r0" narrowing, the far band) is in absolute time Tmin, not in distance from the seeds: for the
 *    reflected continuation of a point-source field that is the right measure of the front's
 *    curvature; a front seeded at t = 0 starts with the narrowed band of a point source.
 * 4. Capacity.  Seeds plus close cells must fit the hand-over's 11 881 entries (109 x 109), else
 *    ALIFMM_E_CAPACITY with a message, decided on the host before any launch.  A 4096-node back wall
 *    on the grid's last row needs 8 192 and fits; a 4096-node interior line needs 12 288 and does not
 *    (seed it in pieces of other calls' fields, or coarser); more entries are not supported.
 * 5. Errors.  ALIFMM_E_ARG with a message, the context staying usable, when: the context has no
 *    model; nfield < 1 or nseed < 1; a node is outside the grid or listed twice; both or neither of
 *    seed_t and from_slot are given; a from_slot is empty, not of subgrid 1, of another shape, or
 *    inside the destination range; a seed time, host or gathered, is not finite or is negative (the
 *    sign bit set: -0.0 too).  A negative Tmin makes the band width negative and nothing is ever
 *    accepted, and the band kernel's edge buffers encode known-ness in the sign of -t; gathered
 *    times are checked on the device, before the band launch.
 * 6. Untouched state.  The seeded hand-overs live in a buffer of their own: the signatures of
 *    "init_reuse" and the hand-overs they vouch for are not touched (a travel call repeated after a
 *    seeded call skips its walks as if nothing had happened in between), alifmm_init_profile keeps
 *    reporting source-init walks only, and the from_slot fields and every slot outside the
 *    destination range are not modified.
 * 7. Around the call.  Chunking by "batch", the work-list capacity retry, "members", "stripe_log",
 *    "xcd_local", alifmm_source_stats, alifmm_band_profile and alifmm_last_timing work as for
 *    alifmm_travel; init_ms is then the seed pass.  The fields are bit-identical for every member
 *    count and chunking, and a field does not depend on the other fields of its call.
 *    alifmm_get_option "cap_scale" (read-only): 1 on a fresh context, x 4 per capacity retry so far.
 * 8. alifmm_get_option: "seed_ms" (uploads and the seed kernel of the last call), "seed_nodes" and
 *    "seed_close" (its seeds and close cells, set also when the call fails with ALIFMM_E_CAPACITY).
 * 9. A seed layer one node thick.  From a flat isotropic front given on one row, fouds18_A() finds
 *    three collinear known nodes and gives the next row t + (2/3) dnz / v (t + dnz / v next to the
 *    side columns, where it sees fewer): the one-layer start is early by a third of a cell's time,
 *    once — 8e-5 of a 4096-cell path, inside the project's 1.4e-3 field envelope.  A consistent layer
 *    two nodes thick continues a plane front exactly (to 1e-15).  Give two layers where they exist
 *    (the reflector row and the row before it, both read from the incident field).  The operators
 *    are the reference's and are not altered. */
int alifmm_travel_seeded(alifmm_ctx* ctx, int nfield, int nseed, const int32_t* seed_iz, const int32_t* seed_ix,
                         const double* seed_t, const int32_t* from_slot, int first_slot, double* out);

/* Copy a resident field to the host; release all resident fields. */
int alifmm_get_field(alifmm_ctx* ctx, int slot, double* out);
int alifmm_release_fields(alifmm_ctx* ctx);

/* Copy the resident fields of slots first_slot .. first_slot+n-1 (one shape) into dst, slot after
 * slot (the (nsrc, fnz, fnx) result stack of ALI_FMM.update() :3870-3936, which the reference's
 * workers return over queue2 :3610, :3659).  dst_kind 0: pageable host memory, copied through a
 * ring of pinned staging buffers (the DMA of one piece overlaps the host copy of the previous);
 * 1: host memory the DMA engine can write directly (pinned or registered); 2: device memory of
 * this context's GPU (e.g. a communication buffer); 3: pageable host memory registered with the
 * DMA engine for the duration of the copy (hipHostRegister), then written directly.
 * *gbps (nullable) = bytes / wall time. */
int alifmm_copy_fields(alifmm_ctx* ctx, int first_slot, int n, double* dst, int dst_kind, double* gbps);

/* Trace npairs rays (replaces find_ray() :3104-3465 incl. ray_time() :2992-3022).
 *   field_slot[k]        resident field of the RECEIVER of ray k (its subgrid is used)
 *   src_xy[2k], rec_xy[2k]  source / receiver (x, z) on that field's fine grid
 *   times[k]             ray travel time [s]; 0 for a ray cut short (flags bit1 or bit2), which the
 *                        reference never times
 *   ray_len[k]           number of points (>= 2)
 *   flags[k]             bit0: reference's early exit ("Travel time to receiver increasing"),
 *                        bit1: point capacity reached, bit2: empty candidate plane
 *   ray_xy (nullable)    packed points: ray k's x at ray_xy[2*off[k] + 2*i], z at +1,
 *                        off[k] = sum of ray_len[0..k-1]; capacity ray_xy_cap points.
 *                        ray_xy == NULL with ray_xy_cap == ALIFMM_KEEP_RAYS keeps the packed
 *                        points in the context for alifmm_take_rays() (exactly sized buffer).  */
#define ALIFMM_KEEP_RAYS (-1)
int alifmm_find_rays(alifmm_ctx* ctx, int npairs, const int32_t* field_slot, const double* src_xy,
                     const double* rec_xy, double* times, int32_t* ray_len, int32_t* flags,
                     double* ray_xy, int64_t ray_xy_cap);

/* Packed points kept by the last alifmm_find_rays(..., NULL, ALIFMM_KEEP_RAYS): *n_points = their
 * count (sum of ray_len); with ray_xy != NULL (capacity ray_xy_cap points) they are copied out in
 * the layout of alifmm_find_rays() and released.  Compact ray storage for full-matrix captures
 * (the reference's dense (n, n, 5(nnz+nnx)) arrays, :4286-4289, do not fit at 4096²). */
int alifmm_take_rays(alifmm_ctx* ctx, double* ray_xy, int64_t ray_xy_cap, int64_t* n_points);

/* Back-wall echo paths between element pairs: element a -> reflector -> element b, the only
 * arrivals that cross the part when one array sits on one face (pulse-echo: a = b).  The reference
 * has no counterpart.  By Fermat and reciprocity the first reflected arrival is the minimum over the
 * reflector nodes w of T_a(w) + T_b(w), the specular point w* is where it is taken, and the path is
 * two back-traced rays, w* -> a through T_a and w* -> b through T_b, joined into one ray a .. w* .. b
 * that alifmm_ray_sens and alifmm_sens_op_build walk as any other.
 *
 * alifmm_skip_pick
 *   slot_a[k], slot_b[k]  int32 [npairs] resident fields of pair k's two elements.  Slots may repeat
 *                      and slot_a[k] == slot_b[k] is allowed; all slots of a call hold fields of one
 *                      subgrid and one shape
 *   w_iz, w_ix         int32 [nw] reflector nodes on the fields' fine grid: any node set in any order;
 *                      a node may be listed twice
 *   pick_time, hit     float64 [npairs], int32 [npairs]
 * For pair k and node q, s_q = T_a[w_iz[q]][w_ix[q]] + T_b[w_iz[q]][w_ix[q]] (one float64 add).  The
 * candidates are the q whose s_q is finite (neither NaN nor +-inf).  hit[k] is the smallest q among
 * those with the least s_q, and pick_time[k] = s_hit[k]; with no candidate hit[k] = -1 and
 * pick_time[k] = +inf.  The result is the minimum of a total order (the sum, then the node number;
 * -0.0 equals 0.0), so it does not depend on how the device reduces.  A pair's result depends on
 * nothing else in the request, and the fields are not modified.  On the device one pass per distinct
 * slot gathers its values at the nodes (a strided reflector is read once per field, not once per
 * pair) into a grow-only buffer of the context, freed with it; one wavefront per pair reduces.
 *
 * alifmm_skip_rays     the pick, then two legs per pair traced by the ray kernel of alifmm_find_rays
 *   a_xy[2k], b_xy[2k] float64 [npairs][2] the elements' (x, z) on the fields' fine grid
 *   pick_time, hit     as above; each nullable here
 *   times, ray_len, flags, ray_xy, ray_xy_cap   as in alifmm_find_rays, for the joined rays
 * Leg A of pair k starts at (w_ix[hit], w_iz[hit]) with receiver a_xy[k] in field slot_a[k]; leg B
 * starts at the same point with receiver b_xy[k] in field slot_b[k].  A leg's points, time and flag
 * bits are those of the same job given to alifmm_find_rays, whatever the chunking and the lanes per
 * ray.  The joined ray is leg A's points in reverse order, then leg B's from its second point on:
 * ray_len = len_A + len_B - 1, the first point is a, the last is b, and the hit node appears once.
 * flags = flags_A | flags_B; bit 3 (value 8): no hit — such a ray has ray_len 0 and times 0 and is
 * not traced.  times[k] = t_A + t_B (one float64 add, in that order), 0 when flags has bit 1 or 2
 * set, as alifmm_find_rays does for a ray cut short.  A joined ray holds up to
 * 2 * 5 * (nnz + nnx) - 1 points.  ray_xy, ray_xy_cap, ALIFMM_KEEP_RAYS, alifmm_take_rays and the
 * ray_xy == NULL forms of alifmm_ray_sens and alifmm_sens_op_build behave exactly as after
 * alifmm_find_rays with the joined rays as the rays (a join kernel writes them where the packing
 * kernel writes kept rays; the kept-point budget and its host staging are unchanged).  The 4-byte
 * hits come to the host to make the leg jobs.
 *
 * Both: npairs == 0 is ALIFMM_OK.  ALIFMM_E_ARG with a message, the context staying usable, when:
 * the context has no model; npairs < 0 or nw < 1; slot_a, slot_b, w_iz or w_ix is NULL, pick_time or
 * hit (skip_pick), a_xy, b_xy, times or ray_len (skip_rays) is NULL; a slot is empty; the slots mix
 * subgrids or shapes; a node lies outside the field; skip_rays: the subgrid's 6 sg + 3 plane
 * candidates exceed what the ray kernel holds (256), or ray_xy holds fewer than the joined rays'
 * points (nothing is written then, as with alifmm_find_rays).  One GPU.
 * alifmm_get_option: "skip_pick_ms" (the gather and pair-reduction kernels of the last call),
 * "skip_join_ms" (the join kernel, summed over the launches), and after alifmm_skip_rays the ray
 * timings as after alifmm_find_rays ("ray_kernel_ms", "find_rays_ms", "ray_lanes"; "ray_pack_ms" 0). */
int alifmm_skip_pick(alifmm_ctx* ctx, int npairs, const int32_t* slot_a, const int32_t* slot_b, int nw,
                     const int32_t* w_iz, const int32_t* w_ix, double* pick_time, int32_t* hit);
int alifmm_skip_rays(alifmm_ctx* ctx, int npairs, const int32_t* slot_a, const int32_t* slot_b, const double* a_xy,
                     const double* b_xy, int nw, const int32_t* w_iz, const int32_t* w_ix, double* pick_time,
                     int32_t* hit, double* times, int32_t* ray_len, int32_t* flags, double* ray_xy,
                     int64_t ray_xy_cap);

/* Diagnostics of the last alifmm_travel(): per slot band steps [stage1, stage2, stage3|-, main]
 * and main-grid cell-sweeps (local-operator evaluations); device time of the last call's kernels. */
int alifmm_source_stats(alifmm_ctx* ctx, int slot, int64_t* steps4, int64_t* cell_sweeps);
int alifmm_last_timing(alifmm_ctx* ctx, double* init_ms, double* band_ms, double* total_ms);

/* Band-kernel profile of a slot's last alifmm_travel() when option "prof" is 1 (zeros otherwise):
 * out14[0..5] wall-clock ticks (100 MHz) spent by the workgroup in the step phases [Tmin, accept,
 * claim, evaluate, fallback, commit]; out14[6..8] sums over steps of the close / accepted /
 * evaluated list sizes; out14[9] the largest close set; out14[10], [11], [13] thread 0's ticks
 * inside phases (wait for the cross-member exchange, neighbour rim-list read, drain before the
 * exchange); out14[12] 100 x the main-loop steps (alifmm_source_stats steps4[3]) whose exchange
 * stored XCD-locally (every member on one XCD; always 0 with option "xcd_local" 0 or one member). */
int alifmm_band_profile(alifmm_ctx* ctx, int slot, int64_t* out14);
/* Wall clock (100 MHz ticks) at which the band kernel's first member of the slot's source started
 * and finished in the last alifmm_travel(): out2[0], out2[1] (dispatch and load-balance diagnostic). */
int alifmm_band_span(alifmm_ctx* ctx, int slot, int64_t* out2);
/* Source-init profile of source i of the last travel chunk (subgrid 1): wall-clock ticks
 * (100 MHz) of stage 1, 2, 3 and the exact main-loop prefix, their heap pops, the ticks the
 * relaxation role was busy in each, and their relaxations | fouds18_A() fallbacks << 32.
 * For a source whose initialisation was skipped (option "init_reuse") this is the profile of the
 * walk that produced its hand-over, in whichever earlier call that ran. */
int alifmm_init_profile(alifmm_ctx* ctx, int i, int64_t* out16);

/* Upload a host travel-time field (fine grid of `subgrid`) into a slot, e.g. for find_ray() on a
 * field computed elsewhere (find_ray's rec_TTF argument, :3105). */
int alifmm_put_field(alifmm_ctx* ctx, int slot, int subgrid, const double* data);

/* Total-focusing-method (TFM) image of full-matrix-capture data, delay-and-sum over resident
 * travel-time fields (the first-arrival delay laws): I(p) = sum_a sum_b w_ab s_ab(T_a(p) + T_b(p)).
 * The fields stay on the device; one image comes back.
 *   subgrid            the fields' subgrid
 *   tx_slot[ntx], rx_slot[nrx]  resident slots of the transmitters' / receivers' fields.  Every
 *                      named slot holds a field of `subgrid` and of one common shape (fnz, fnx);
 *                      slots may repeat, the lists may overlap or be the same array
 *   fmc                float32 [ntx][nrx][nt][ncomp]; ncomp 1: real RF, 2: analytic signal, re and
 *                      im interleaved
 *   t0, fs             time [s] of sample 0, sampling rate [Hz]
 *   pair_w (nullable)  float32 [ntx][nrx] (apodisation, or a trans_pairs-style 0/1 mask)
 *   iz0, ix0, niz, nix, step  pixel window on the fields' fine grid: pixel (i, j) is node
 *                      (iz0 + step i, ix0 + step j).  Pixels are field nodes: no spatial
 *                      interpolation of T is defined or needed
 *   image              float64 [niz][nix][ncomp]
 * One term (a, b) at pixel p, all in float64, operations in this order, no contraction:
 *   1. w = pair_w ? (double)pair_w[a][b] : 1.0; if w == 0 the term is 0
 *   2. u = ((T_a(p) + T_b(p)) - t0) * fs
 *   3. the term is 0 unless u >= 0 && u < nt - 1 (written so that NaN, +-inf and huge values fail
 *      it; made before any conversion to an integer)
 *   4. k = (int64)u, f = u - (double)k
 *   5. x0 = (double)fmc[a][b][k], x1 = (double)fmc[a][b][k+1], per component
 *   6. term = w * (x0 + f * (x1 - x0))
 * I(p) = the float64 sum of the terms in an order that is fixed per pixel (it depends on ntx, nrx
 * and option "tfm_chunk" only, not on the window, the step or the pixel's place in a tile): the
 * same pixel computed through two windows has the same bits.
 * ALIFMM_E_ARG with a message, the context staying usable, when: the context has no model; a slot
 * is empty; the slots mix subgrids or shapes; ntx or nrx < 1 or nt < 2; ncomp is not 1 or 2; fs
 * is not finite and positive or t0 is not finite; step, niz or nix < 1; the window reaches outside
 * the field; tx_slot, rx_slot, fmc or image is NULL.
 * The fields in the slots are not modified.  All offsets into fmc are 64-bit (ntx nrx nt ncomp
 * passes 2^31 at realistic sizes).  The data, the weights, the slot pointer table and the image
 * live in grow-only device buffers of the context, freed with it.  alifmm_get_option:
 * "tfm_upload_ms" (host -> device copies) and "tfm_kernel_ms" (the kernel) of the last call;
 * alifmm_set_option "tfm_chunk" (4, 8, 16 or 32, default 8): receivers whose delays a pixel keeps
 * in registers per pass over the transmitters (changes the summation order, so the last bits). */
int alifmm_tfm(alifmm_ctx* ctx, int subgrid, int ntx, const int32_t* tx_slot, int nrx, const int32_t* rx_slot,
               const float* fmc, int nt, int ncomp, double t0, double fs, const float* pair_w, int iz0, int ix0,
               int niz, int nix, int step, double* image);

/* FMC modelling: the full-matrix-capture data a reflectivity map predicts under the delay laws of
 * resident travel-time fields; the exact transpose of alifmm_tfm, term by term.  The fields stay on
 * the device; the modelled data come back.
 *   subgrid, tx_slot[ntx], rx_slot[nrx], t0, fs, pair_w, ncomp, iz0, ix0, niz, nix, step
 *                      as in alifmm_tfm
 *   refl               float64 [niz][nix][ncomp] on the pixel window (pixel (i, j) is node
 *                      (iz0 + step i, ix0 + step j)); every value finite
 *   fmc_out            float64 [ntx][nrx][nt][ncomp]
 * For every pixel p whose components are not all zero and every pair (a, b), all in float64,
 * operations in this order, no contraction:
 *   1. w = pair_w ? (double)pair_w[a][b] : 1.0; if w == 0 there is no term
 *   2. u = ((T_a(p) + T_b(p)) - t0) * fs
 *   3. there is no term unless u >= 0 && u < nt - 1 (the test of alifmm_tfm step 3, made before
 *      any conversion to an integer)
 *   4. k = (int64)u, f = u - (double)k
 *   5. per component c: g = w * refl[p][c], c1 = f * g, c0 = g - c1
 *   6. the term adds c0 to fmc_out[a][b][k][c] and c1 to fmc_out[a][b][k+1][c]
 * fmc_out[a][b][k][c] is the float64 sum of what the terms add to it, starting from +0.0.  The
 * order of that sum is NOT fixed: the result is reproducible to rounding only, as the maps of
 * alifmm_ray_sens are.  A sample that receives exactly one contribution has exactly that value, a
 * sample that receives none is +0.0.  A pixel whose components are all +-0 contributes nothing and
 * costs no field read (the map is compacted on the host, only its non-zero pixels are uploaded).
 * The set of terms is exactly that of alifmm_tfm for the same slots, window, step, t0, fs, nt and
 * weights, and the map is the transpose of that linear map: <tfm(d), x> = <d, model(x)> to
 * rounding, component-wise.
 * ALIFMM_E_ARG with a message, the context staying usable and nothing written to fmc_out: every
 * condition of alifmm_tfm (refl / fmc_out in place of fmc / image), and a non-finite value in refl.
 * The fields in the slots are not modified.  All offsets are 64-bit.  The non-zero pixels, the
 * weights, the slot pointer table and the output live in grow-only device buffers of the context,
 * freed with it.  alifmm_get_option: "tfm_model_upload_ms" (compaction and host -> device copies)
 * and "tfm_model_kernel_ms" (zeroing and kernel) of the last call.  alifmm_set_option:
 * "tfm_model_tile": samples of a trace a workgroup accumulates in LDS per pass (0, the default:
 * the whole trace, at most what 128 KiB of LDS hold for two traces; larger values are cut to that);
 * "tfm_model_slabs": slabs of the non-zero pixels per trace group, 0 (automatic) or 1 .. 64, cut to
 * the number of non-zero pixels; with more than one the slabs' tiles are added into the zeroed
 * output with float64 atomics; "tfm_model_rx": receivers of one transmitter per workgroup, 1, 2
 * (default) or 4 (the LDS is shared by their traces, so the largest tile shrinks accordingly);
 * "tfm_model_combine": 0 .. 64, default 12: a wave whose lanes fall into at most this many runs of
 * neighbouring lanes that add to the same sample sums each run before its LDS atomics (0: never;
 * another summation order, the same contract).  Read-only "tfm_model_tile_used" and
 * "tfm_model_slabs_used": what the last call ran with (reading the settings back gives the
 * settings, 0 for automatic).  One GPU. */
int alifmm_tfm_model(alifmm_ctx* ctx, int subgrid, int ntx, const int32_t* tx_slot, int nrx, const int32_t* rx_slot,
                     const double* refl, int ncomp, int nt, double t0, double fs, const float* pair_w, int iz0, int ix0,
                     int niz, int nix, int step, double* fmc_out);

/* alifmm_tfm on float64 data: the same signature and contract with fmc float64
 * [ntx][nrx][nt][ncomp], the same term (steps 1 - 6, x0 and x1 read as they are), the same
 * per-pixel summation order (a function of ntx, nrx and "tfm_chunk" only), the same errors.  Two
 * consequences are part of the contract: on data whose every value float32 represents exactly the
 * image has the bits of alifmm_tfm on those float32 data at the same "tfm_chunk"; and the image is
 * bit-reproducible.  This is the A^T of an iterative method, whose residual d - A x is float64:
 * alifmm_tfm would truncate it, and the pair would stop being A / A^T at about 6e-8.
 * "tfm_upload_ms", "tfm_kernel_ms" and "tfm_chunk" are alifmm_tfm's (one option, one default). */
int alifmm_tfm_f64(alifmm_ctx* ctx, int subgrid, int ntx, const int32_t* tx_slot, int nrx, const int32_t* rx_slot,
                   const double* fmc, int nt, int ncomp, double t0, double fs, const float* pair_w, int iz0, int ix0,
                   int niz, int nix, int step, double* image);

/* Coherence-weighted TFM: alifmm_tfm's image together with a per-pixel factor in [0, 1] that says
 * how well the aperture's contributions agree, from a second sum over the same terms made inside
 * the same delay-and-sum.  The fields stay on the device; the image, the factor and, if asked for,
 * the raw sums come back.  The exponent and the product image * factor^p are the caller's.
 *   subgrid ... step   as in alifmm_tfm (fmc float32)
 *   kind               1 the coherence factor (CF), 2 the sign coherence factor (SCF), 3 the phase
 *                      (circular) coherence factor (PCF; ncomp 2 only)
 *   image              float64 [niz][nix][ncomp]
 *   factor             float64 [niz][nix]
 *   sums (nullable)    float64 [niz][nix][3]: the raw sums of `kind`
 * A counting term is a term (a, b) that passes steps 1 and 3 of alifmm_tfm (w != 0 and
 * 0 <= u < nt - 1); t_c is its value of step 6 for component c.  A counting term whose value is 0
 * counts.  Per pixel, all in float64, operations in the order written, no contraction, sqrt and /
 * correctly rounded:
 *   S_c = sum of t_c: image[p][c].  n = the number of counting terms.
 *   kind 1: per term e = t_0 * t_0; if ncomp == 2: e = e + t_1 * t_1; q += e.
 *           num = S_0 * S_0 (if ncomp == 2: + S_1 * S_1), den = n * q,
 *           F = den > 0 ? num / den : 0.                               sums = (n, q, 0)
 *   kind 2: per term b += (t_0 > 0) - (t_0 < 0) (component 0, the RF part).
 *           m = b / n, y = 1 - m * m, F = n > 0 ? 1 - sqrt(y) : 0.     sums = (n, b, 0)
 *   kind 3: per term e as in kind 1, g = sqrt(e); if g > 0: r = 1.0 / g, ph_c += t_c * r; where
 *           g > 0 fails (g is 0 or NaN) the term adds nothing to ph and still counts in n.
 *           num = ph_0 * ph_0 + ph_1 * ph_1, y = 1 - num / (n * n); if y < 0: y = 0;
 *           F = n > 0 ? 1 - sqrt(y) : 0.                               sums = (n, ph_0, ph_1)
 *   factor[p] = F.
 * Every sum runs in alifmm_tfm's per-pixel order (a function of ntx, nrx and "tfm_chunk" only), so
 * image has the bits of alifmm_tfm on the same call, and all three outputs are bit-reproducible and
 * independent of the window, the step and the pixel's place in a tile.  n and b are exact integers,
 * the same for every "tfm_chunk".  Non-finite data give non-finite values at the pixels they
 * reach, as in alifmm_tfm.
 * ALIFMM_E_ARG with a message, the context staying usable and nothing written: every condition of
 * alifmm_tfm; kind outside 1 .. 3; kind 3 with ncomp != 2; image or factor NULL.
 * The fields in the slots are not modified.  The data, the weights, the slot pointer table and the
 * image use alifmm_tfm's device buffers; the factor and the sums live in grow-only device buffers of
 * the context, freed with it.  alifmm_get_option: "tfm_coh_upload_ms" (host -> device copies) and
 * "tfm_coh_kernel_ms" (the kernel) of the last call.  "tfm_chunk" applies as it does to alifmm_tfm.
 * One GPU. */
int alifmm_tfm_coh(alifmm_ctx* ctx, int subgrid, int ntx, const int32_t* tx_slot, int nrx, const int32_t* rx_slot,
                   const float* fmc, int nt, int ncomp, double t0, double fs, const float* pair_w, int iz0, int ix0,
                   int niz, int nix, int step, int kind, double* image, double* factor, double* sums);

/* Least-squares imaging: min |A x - d|^2 + damp^2 |x|^2 + smooth^2 |D x|^2 by CGLS from x = 0, the
 * imaging counterpart of alifmm_sens_op_solve.  The data, every vector and every scalar stay on the
 * device; one image comes back.  The call is stateless like alifmm_tfm: the slots are resolved and
 * validated at call time, there is no resident operator.
 *   subgrid, tx_slot[ntx], rx_slot[nrx], nt, ncomp, t0, fs, pair_w, iz0, ix0, niz, nix, step
 *                      as in alifmm_tfm
 *   fmc                the data d, float64 [ntx][nrx][nt][ncomp], every value finite
 *   image              x, float64 [niz][nix][ncomp]
 *   resid (nullable)   the recurred residual r at the end, the shape of fmc
 *   info8              iterations, sqrt(gamma_0), sqrt(gamma) at the end, |d|, the recurred |r| at the
 *                      end, the stop's reason (0 tol, 1 max_iter, 2 breakdown), 0, 0
 * A is the linear map of alifmm_tfm_model for these slots, window, step, t0, fs, nt and weights, on
 * the dense window and component-wise; it is a real operator (a complex map is two real unknowns
 * per pixel).  A zero pixel takes part as any other pixel: it adds zeros.  A^T is alifmm_tfm_f64.
 * D is the first difference between 4-neighbour pixels of the window, per component:
 * (D^T D p)[q] = sum over the neighbours q' of (p[q] - p[q']), upper, left, right, lower, in that
 * order.  The iteration is alifmm_sens_op_solve's, word for word, with R(v) = damp^2 v +
 * smooth^2 D^T D v:
 *   r = d; s = A^T r; p = s; gamma_0 = gamma = |s|^2; gamma_0 == 0: stop (breakdown)
 *   iteration it = 1, 2, ...:
 *     q = A p; qq = |q|^2 + p . R(p); qq == 0: stop (breakdown; the iteration does not count)
 *     alpha = gamma / qq; x += alpha p; r -= alpha q
 *     s = A^T r - R(x); gamma' = |s|^2; beta = gamma' / gamma; p = s + beta p; gamma = gamma'
 *     gamma <= tol^2 gamma_0: stop (tol); it == max_iter: stop (max_iter)
 * The host reads 8 bytes per iteration for the stop rule.  Every dot product is a two-stage sum
 * whose partial sums depend on the vector's length alone, and A^T has a fixed order; A sums with
 * atomics in no fixed order (as alifmm_tfm_model does).  So a solve is reproducible to rounding
 * only, NOT to the bit, and its iteration count may differ by one between two runs when gamma
 * passes the threshold within rounding.  damp is absolute: |A|_2 is of the order sqrt(ntx nrx).
 * ALIFMM_E_ARG with a message, the context staying usable and nothing written: every condition of
 * alifmm_tfm; a non-finite value in fmc; damp or smooth negative or not finite; max_iter < 1; tol
 * negative or not finite; image or info8 NULL.  A failed device allocation returns ALIFMM_E_HIP
 * with the call's buffers freed.  The fields in the slots are not modified.  All offsets are 64-bit.
 * The vectors (two of the data's size, four of the image's) and the pixel list live in grow-only
 * device buffers of the context, freed with it.  alifmm_get_option: "tfm_lsq_upload_ms" (host ->
 * device copies), "tfm_lsq_kernel_ms" (device time of the whole solve) and "tfm_lsq_iters" of the
 * last call.  "tfm_chunk" and the "tfm_model_*" options apply as they do to the two kernels
 * ("tfm_model_slabs" automatic counts every pixel of the window; with more than one slab q is
 * zeroed every iteration).  One GPU. */
int alifmm_tfm_lsq(alifmm_ctx* ctx, int subgrid, int ntx, const int32_t* tx_slot, int nrx, const int32_t* rx_slot,
                   const double* fmc, int nt, int ncomp, double t0, double fs, const float* pair_w, int iz0, int ix0,
                   int niz, int nix, int step, double damp, double smooth, int max_iter, double tol, double* image,
                   double* resid, double* info8);

/* The trace FIR P and its exact transpose P^T: every trace convolved with one pulse (transpose:
 * correlated with it), on the device in a fixed order.  Measured FMC data are the spike trains of
 * alifmm_tfm_model convolved with the transducer's pulse; P is that step as a linear operator.
 *   in                 float64 [ntrace][nt][ncomp], ncomp 1 (real) or 2 (re, im interleaved)
 *   taps               the pulse h, float64 [ntap][tap_comp]: tap_comp 1 real taps, applied to each
 *                      component; 2 complex taps (re, im), ncomp 2 only; every value finite
 *   origin             the tap index of the pulse's time zero, 0 <= origin < ntap (0: a causal pulse,
 *                      out[k] = sum_j h[j] in[k - j])
 *   transpose          0: out = P in; 1: out = P^T in
 *   out                float64, the shape of in; may be in itself
 * Per trace and output sample t, all in float64, operations in the order written, no contraction:
 *   forward    y[t] = sum over j = 0 .. ntap - 1, ascending, of h[j] * x[t - j + origin]
 *   transpose  z[t] = sum over j ascending of conj(h[j]) * y[t + j - origin]
 *   the accumulator starts at +0.0 per component; a sample index outside 0 .. nt - 1 adds nothing
 *   real tap     acc_c += h * x_c (one multiply, one add) for each component c
 *   complex tap  pr = (hr * xr) - (hi * xi); pi = (hr * xi) + (hi * xr); acc_r += pr; acc_i += pi;
 *                the transpose negates hi first
 * So the outputs are bit-reproducible, a trace's result does not depend on the other traces of the
 * call, and <P x, y> = <x, P^T y> to rounding under the real inner product (P^T is the transpose of
 * the real matrix of P on interleaved components).  The data are not checked: a non-finite sample
 * propagates to the outputs it reaches.
 * ALIFMM_E_ARG with a message, the context staying usable and nothing written: ctx, in, taps or out
 * NULL; ntrace < 1; nt < 1; ncomp or tap_comp not 1 or 2; tap_comp 2 with ncomp 1; ntap < 1 or
 * ntap > ALIFMM_FIR_MAX_TAPS; origin outside [0, ntap); a non-finite tap; transpose not 0 or 1.
 * Needs no model.  Upload, one kernel, download; the traces and the taps live in grow-only device
 * buffers of the context, freed with it.  All trace offsets are 64-bit.  alifmm_get_option:
 * "trace_fir_upload_ms" (host -> device copies) and "trace_fir_kernel_ms" (the kernel) of the last
 * call; "trace_fir_tile", the output samples a workgroup makes (a constant of the build: the results
 * do not depend on it).  One GPU. */
#define ALIFMM_FIR_MAX_TAPS 1024
int alifmm_trace_fir(alifmm_ctx* ctx, int64_t ntrace, int nt, int ncomp, const double* in, int ntap, int tap_comp,
                     const double* taps, int origin, int transpose, double* out);

/* The spectral trace filter: y = IDFT(G · DFT(x)) per trace on the device, G the analytic mask, the
 * caller's frequency response, or both, in a fixed order of operations.  It makes real RF analytic
 * (scipy.signal.hilbert's definition) and band-passes it in the same pass, which the imaging entry
 * points expect of their complex data.
 *   in                 [ntrace][nt][ncomp], ncomp 1 (real) or 2 (re, im interleaved)
 *   dtype              0 float64, 1 float32: of in and of out
 *   nfft               the transform length N: a power of two, nt <= N <= ALIFMM_FFT_MAX; 0: the
 *                      smallest power of two >= nt
 *   resp_comp, resp    0 and NULL: no response; else float64 [N][resp_comp], real (1) or complex (2):
 *                      H_k at DFT bin k in numpy's bin order; every value finite
 *   analytic           1: the mask m_0 = 1, m_{N/2} = 1 (N >= 2), m_k = 2 for 0 < k < N/2, 0 above
 *                      (scipy.signal.hilbert(x, N=nfft)); 0: none
 *   out                complex, [ntrace][nt][2], of the same dtype; may not be in
 * Per trace, all in float64, operations in the order written, no contraction:
 *   load      v[n] = x[n] for n < nt (a float32 sample converts exactly; a real sample gets
 *             im = +0.0), (+0.0, +0.0) for nt <= n < N
 *   twiddles  W_N^m = (c_m, -s_m), c_m = cos(2 pi m / N), s_m = sin(2 pi m / N) of the exact real
 *             argument, each rounded once to nearest: the committed table csrc/fft_twiddles.h holds
 *             sin(2 pi m / 8192), m = 0 .. 2048; the other quadrants and the cosines follow by exact
 *             symmetry, and a smaller N reads the table with the stride 8192 / N (the same real
 *             number, so the same bits)
 *   product   a · w = ((ar * wr) - (ai * wi), (ar * wi) + (ai * wr)): each product rounded, then
 *             the subtraction and the addition
 *   forward   radix-2 decimation in frequency, in place: for l = 0 .. log2 N - 1, half = N >> (l+1),
 *             every block of 2 half elements and i < half: a = v[p], b = v[p + half], v[p] = a + b,
 *             d = a - b, v[p + half] = d · W_N^(i << l).  X_k now lies at v[bitrev(k)].
 *   pointwise at v[bitrev(k)]: a complex H_k multiplies by the product above (w = H_k), a real one
 *             scales both components; then the mask: (vr * 2, vi * 2) for 0 < k < N/2, (+0.0, +0.0)
 *             for k > N/2, and nothing for m_k = 1 (the product with 1 changes no bit)
 *   inverse   radix-2 decimation in time, from the bit-reversed order back to natural order: for
 *             l = log2 N - 1 .. 0, the same pairs: a = v[p], b = v[p + half] · conj(W_N^(i << l)),
 *             v[p] = a + b, v[p + half] = a - b
 *   store     y[n] = (vr * (1 / N), vi * (1 / N)) for n < nt: the scaling is exact; rounded once to
 *             float32 for dtype 1
 * Every butterfly multiplies by its twiddle, W^0 = (1, -0) included: no product is skipped, in the
 * kernel, in the numpy restatement (tests/trace_fft_ref.py) and in the host replay
 * (tests/trace_fft_sim.cpp).  There is no permutation pass: the forward transform leaves the
 * bit-reversed order and the inverse consumes it.  The kernel groups up to three layers into one
 * pass over registers; an element still sees exactly these operations in this order.
 * So a trace's result depends on nothing but that trace, N, resp and analytic, and is
 * bit-reproducible between calls.  The data are not checked: a non-finite sample makes that trace's
 * output unspecified and leaves the other traces alone.
 * ALIFMM_E_ARG with a message, the context staying usable and out untouched: ctx, in or out NULL;
 * out == in; ntrace < 1; nt < 1 or nt > ALIFMM_FFT_MAX; ncomp not 1 or 2; dtype not 0 or 1; nfft not
 * 0 and not a power of two in [nt, ALIFMM_FFT_MAX]; resp_comp not 0, 1 or 2; resp NULL with
 * resp_comp > 0 or given with resp_comp 0; a non-finite response value; analytic not 0 or 1; more
 * traces than 64-bit byte offsets hold.
 * Needs no model.  Upload, one kernel, download; the traces and the response live in grow-only
 * device buffers of the context, freed with it.  All trace offsets are 64-bit.  alifmm_get_option:
 * "trace_fft_upload_ms" (host -> device copies), "trace_fft_kernel_ms" (the kernel) and
 * "trace_fft_download_ms" (the device -> host copy) of the last call; "trace_fft_grid", the most
 * workgroups a launch starts (a constant of the build; a workgroup transforms
 * max(1, min(512, 2048 / N)) traces at a time and walks the rest with the grid's stride).  One GPU. */
#define ALIFMM_FFT_MAX 8192
int alifmm_trace_spectral(alifmm_ctx* ctx, int64_t ntrace, int nt, int ncomp, int dtype, const void* in, int nfft,
                          int resp_comp, const double* resp, int analytic, void* out);

/* Time-of-flight picks: per trace the peak of the envelope inside a gate, or its onset, refined to a
 * fraction of a sample, with the runner-up as a measure of ambiguity; on the device, from traces the
 * caller holds, optionally through alifmm_trace_spectral's filter without the filtered traces ever
 * leaving the device.  It makes the measured times the inversion entry points take
 * (measured - computed).
 *   in                 [ntrace][nt][ncomp], ncomp 1 (real) or 2 (re, im interleaved)
 *   dtype              0 float64, 1 float32
 *   filter             0: pick on in as given; nfft, resp_comp and analytic must be 0 and resp NULL.
 *                      1: pick on what alifmm_trace_spectral(ntrace, nt, ncomp, dtype, in, nfft,
 *                      resp_comp, resp, analytic) returns (complex, of the same dtype), with its
 *                      limits (nt <= ALIFMM_FFT_MAX); the picks are, to the bit, those of filter 0 on
 *                      that output
 *   gate_lo, gate_hi   int32 [ntrace]: the trace's gate, samples lo <= n < hi; 0 <= lo and hi <= nt;
 *                      lo >= hi: the trace is not asked for
 *   mode               0 peak, 1 onset
 *   frac               mode 1: the onset's threshold as a fraction of the peak amplitude, 0 < frac <= 1
 *   guard              >= 0: the runner-up lies more than guard samples from the peak
 *   pos, amp, amp2     float64 [ntrace]: the pick in samples (seconds: t0 + pos / fs), the peak's and
 *                      the runner-up's amplitude
 *   idx, idx2, flags   int32 [ntrace]: the peak's and the runner-up's sample, the flags below
 * Per trace, all in float64, operations in the order written, no contraction (x the picked traces:
 * in, or the filter's output):
 *   energy     e[n] = (re * re) + (im * im), x * x for real data; a float32 sample converts exactly
 *   candidate  a sample of the gate whose e is neither NaN nor +-inf (a test on the bits).  Any other
 *              sample in the gate sets flag 16 and is not picked
 *   peak       idx = the maximum over the gate's candidates of the total order "larger e first, of
 *              equal e the lower n"; amp = sqrt(e[idx]), correctly rounded.  No candidate, or
 *              e[idx] == 0: flag 2, idx = idx2 = -1, pos = NaN, amp = amp2 = 0, nothing else
 *   runner-up  idx2 = the maximum of the same order over the gate's candidates with
 *              |n - idx| > guard; amp2 = sqrt(e[idx2]); none: idx2 = -1, amp2 = 0.  A maximum, so no
 *              summation order enters; amp2 / amp near 1 marks a cycle skip or a second echo
 *   mode 0     m = idx.  If 0 < m < nt - 1 and e[m - 1] and e[m + 1] are neither NaN nor +-inf (they
 *              may lie outside the gate): a- = sqrt(e[m - 1]), a0 = amp, a+ = sqrt(e[m + 1]); if
 *              a- <= a0, a+ <= a0 and den = (a- - (2 * a0)) + a+ < 0: delta = (0.5 * (a- - a+)) / den
 *              (the vertex of the parabola through the three amplitudes).  In every other case
 *              delta = 0 and flag 4.  Flag 8 if m == lo or m == hi - 1 (the gate cut the echo)
 *   mode 1     thr = (frac * frac) * e[idx]; m = the lowest candidate n of the gate with e[n] >= thr
 *              (idx is one).  If m > 0, e[m - 1] is neither NaN nor +-inf and e[m - 1] < thr:
 *              at = sqrt(thr), am = sqrt(e[m]), a- = sqrt(e[m - 1]), den = am - a-; if den > 0:
 *              delta = -((am - at) / den) (where the line through the two amplitudes meets the
 *              threshold).  In every other case delta = 0 and flag 4.  Flag 8 if m == lo
 *   position   pos = (double)m + delta
 *   no gate    lo >= hi: flag 1 alone, the outputs as under flag 2
 * flags: 1 no gate, 2 nothing to pick, 4 unrefined, 8 at the gate's edge, 16 a non-finite sample in
 * the gate.  The two combines of the reduction (the maximum of two keys, the lower of two indices;
 * csrc/trace_pick_term.h) are associative and commutative, so a trace's picks depend on nothing but
 * that trace, its gate and mode, frac, guard, and are bit-reproducible between calls.  The numpy
 * restatement is tests/trace_pick_ref.py, the host replay of the kernel's code
 * tests/trace_pick_sim.cpp.
 * ALIFMM_E_ARG with a message, the context staying usable and no output written: a NULL pointer
 * (resp excepted); ntrace < 1; nt < 1; ncomp not 1 or 2; dtype, filter or mode not 0 or 1; frac
 * outside (0, 1] in mode 1; guard < 0; a gate with lo < 0 or hi > nt; more traces than 64-bit byte
 * offsets hold; filter 0 with nfft, resp_comp or analytic not 0 or resp given; filter 1: every
 * refusal of alifmm_trace_spectral.
 * Needs no model.  Upload, the filter's kernel (filter 1), one pick kernel, a download of 36 bytes
 * per trace; the traces live in alifmm_trace_spectral's grow-only device buffers, the gates and the
 * outputs in three more, freed with the context.  All trace offsets are 64-bit.
 * alifmm_get_option, of the last call: "trace_pick_upload_ms" (host -> device copies),
 * "trace_pick_filter_ms" (the filter's kernel; 0 with filter 0), "trace_pick_kernel_ms" (the pick
 * kernel), "trace_pick_download_ms" (the device -> host copies); "trace_pick_grid", the most
 * workgroups a launch starts (a constant of the build; a workgroup picks 4 traces at a time, one
 * per wavefront, and walks the rest with the grid's stride).  One GPU. */
int alifmm_trace_pick(alifmm_ctx* ctx, int64_t ntrace, int nt, int ncomp, int dtype, const void* in, int filter, int nfft,
                      int resp_comp, const double* resp, int analytic, const int32_t* gate_lo, const int32_t* gate_hi,
                      int mode, double frac, int guard, double* pos, double* amp, int32_t* idx, double* amp2,
                      int32_t* idx2, int32_t* flags);

/* Pulse-aware least-squares imaging: alifmm_tfm_lsq with the pulse in the operator,
 * min |P A x - d|^2 + damp^2 |x|^2 + smooth^2 |D x|^2 by CGLS from x = 0.
 *   subgrid ... tol    as in alifmm_tfm_lsq
 *   ntap, tap_comp, taps, origin
 *                      the pulse, as in alifmm_trace_fir
 *   image, resid, info8
 *                      as in alifmm_tfm_lsq
 * The contract is alifmm_tfm_lsq's, word for word, with P A in place of A and A^T P^T in place of
 * A^T: A and A^T as there, P (alifmm_trace_fir) acting on each of the ntx nrx traces of nt samples.
 *   r = d; s = A^T (P^T r); p = s; gamma_0 = gamma = |s|^2; gamma_0 == 0: stop (breakdown)
 *   iteration it = 1, 2, ...:
 *     q = P (A p); qq = |q|^2 + p . R(p); qq == 0: stop (breakdown; the iteration does not count)
 *     alpha = gamma / qq; x += alpha p; r -= alpha q
 *     s = A^T (P^T r) - R(x); gamma' = |s|^2; beta = gamma' / gamma; p = s + beta p; gamma = gamma'
 *     gamma <= tol^2 gamma_0: stop (tol); it == max_iter: stop (max_iter)
 * resid is the recurred d - P A x; info8 keeps its meaning, sqrt(gamma_0) being |A^T P^T d|.  P and
 * P^T have a fixed order and add no new source of non-reproducibility; A sums with atomics as
 * before, so a solve is reproducible to rounding only.
 * ALIFMM_E_ARG with a message, the context staying usable and nothing written: every condition of
 * alifmm_tfm_lsq; taps NULL; tap_comp not 1 or 2; tap_comp 2 with ncomp 1; ntap < 1 or
 * ntap > ALIFMM_FIR_MAX_TAPS; origin outside [0, ntap); a non-finite tap.  A failed device
 * allocation returns ALIFMM_E_HIP with the call's buffers freed.
 * The vectors are alifmm_tfm_lsq's and one more of the data's size (three instead of two): A writes
 * it and P reads it, P^T writes it and A^T reads it; with more than one slab it is what is zeroed
 * every iteration.  The options and the "tfm_lsq_*" read-outs are alifmm_tfm_lsq's.  One GPU. */
int alifmm_tfm_lsq_pulse(alifmm_ctx* ctx, int subgrid, int ntx, const int32_t* tx_slot, int nrx,
                         const int32_t* rx_slot, const double* fmc, int nt, int ncomp, double t0, double fs,
                         const float* pair_w, int iz0, int ix0, int niz, int nix, int step, double damp, double smooth,
                         int max_iter, double tol, int ntap, int tap_comp, const double* taps, int origin, double* image,
                         double* resid, double* info8);

/* Sparsity-regularised imaging: the minimiser of
 *   F(x) = 1/2 |P A x - d|^2 + 1/2 damp^2 |x|^2 + 1/2 smooth^2 |D x|^2 + lam sum over pixels p of |x_p|
 * by FISTA with backtracking and gradient restart from x = 0, everything resident on the device.
 *   subgrid ... tol    as in alifmm_tfm_lsq_pulse (A, D, damp, smooth, the slots, window, step, t0,
 *                      fs, weights, ncomp)
 *   ntap, tap_comp, taps, origin
 *                      the pulse, as in alifmm_trace_fir; ntap 0 with taps NULL: no pulse, P = I
 *   lam                the weight of the l1 term, in the units of the gradient A^T P^T d (note the 1/2);
 *                      negative: -lam is relative to lam_max (below), lam = -lam * lam_max
 *   lipschitz          L, an estimate of |B^T B + R|_2; 0: the power estimate below
 *   power_iters        rounds of the power estimate (lipschitz 0 only)
 *   restart            1: gradient restart, 0: none
 *   image              x, float64 [niz][nix][ncomp]: the last accepted x+, never y
 *   resid (nullable)   d - P A x of the returned x, computed from it, not recurred; the shape of fmc
 *   info12             iterations (accepted), G0 = |g0|, the last Gk, |d|, |d - B x|, the stop's reason
 *                      (0 tol, 1 max_iter, 2 breakdown), lam_max, the lam used, the final L, backtracks,
 *                      restarts, the non-zero pixels of x
 * |x_p| is the modulus of pixel p over its components: |x| for ncomp 1, sqrt(re^2 + im^2) for ncomp 2
 * (a complex pixel is one group; its phase is not penalised).  lam_max = max_p |(A^T P^T d)_p| is the
 * smallest lam for which x = 0 is the minimiser.  With B = P A, R(v) = damp^2 v + smooth^2 D^T D v and
 * f(v) = 1/2 |B v - d|^2 + 1/2 v . R(v), all in float64, no contraction, sqrt and / correctly rounded:
 *   g0 = B^T d; G0 = |g0|; lam_max = max_p |g0_p|; G0 == 0: stop (breakdown), x = 0
 *   L = lipschitz > 0 ? lipschitz : the power estimate: v = g0 / |g0|; power_iters times
 *       w = B^T (B v) + R(v), est = |w|, v = w / est; L = est (not finite or 0: stop, breakdown)
 *   x = y = 0; B x = 0; theta = 1; g = -g0; fy = 1/2 |d|^2
 *   iteration k = 1, 2, ...:            (g = B^T r + R(y) with r = B y - d, fy = 1/2 |r|^2 + 1/2 y . R(y))
 *     repeat:
 *       step = 1 / L; tau = lam * step
 *       per pixel: z_c = y_c - step * g_c; m = |z|;
 *                  m > tau: fac = (m - tau) / m, x+_c = z_c * fac; else x+_c = +0.0
 *       B x+ by the two kernels; f+ = 1/2 |B x+ - d|^2 + 1/2 x+ . R(x+)
 *       Q = (fy + g . (x+ - y)) + (1/2 L) |x+ - y|^2
 *       f+ <= Q + 2^-40 fy: accept; else L = 2 L, backtracks += 1
 *       (more than 60 doublings in one call: stop, breakdown; the image is the last accepted x+)
 *     Gk = L |x+ - y|                              (the norm of the gradient mapping)
 *     restart != 0 and (y - x+) . (x+ - x) > 0: theta = 1, restarts += 1
 *     theta+ = (1 + sqrt(1 + 4 theta^2)) / 2; beta = (theta - 1) / theta+; theta = theta+
 *     Gk <= tol G0: stop (tol); k == max_iter: stop (max_iter)
 *     y = x+ + beta (x+ - x); r = (B x+ + beta (B x+ - B x)) - d; x = x+; B x = B x+
 *     fy and g for the new y
 * B y is never computed: one A and one A^T (and the two FIR passes) run per accepted iteration, as in
 * a CGLS iteration, and one more A (and P) per rejected trial.  2^-40 is a constant of the contract: it
 * keeps the rounding of f+ and Q from doubling L once x+ is y to rounding.  The power estimate is a
 * lower bound of the true constant, which is why the backtracking is not optional.  The host reads
 * 32 bytes in one copy per trial (f+, Q + 2^-40 fy, |x+ - y|^2, the restart's dot product), 24 at the
 * start, 8 after the power estimate and 16 at the end.  Every sum is a two-stage sum whose partial
 * sums depend on the vector's length alone (the sums of one pass side by side), lam_max is a maximum
 * and does not depend on an order, A^T and P have a fixed order; A sums with atomics, so a solve is
 * reproducible to rounding only, NOT to the bit, exactly as alifmm_tfm_lsq.
 * ALIFMM_E_ARG with a message, the context staying usable and nothing written: every condition of
 * alifmm_tfm_lsq_pulse (the taps' only with a pulse); lam not finite; lipschitz negative or not
 * finite; power_iters < 1 with lipschitz 0; restart not 0 or 1; info12 NULL.  A failed device
 * allocation returns ALIFMM_E_HIP with the call's buffers freed.  The fields are not modified.
 * The vectors live in grow-only device buffers of the context, freed with it: four of the data's size
 * (d, B x, B x+, r; a fifth between P and A with a pulse) and five of the image's (x, x+, y, g and
 * t = B^T r), and the pixel list.  alifmm_get_option: "tfm_sparse_upload_ms", "tfm_sparse_kernel_ms"
 * (device time of the whole solve), "tfm_sparse_iters", "tfm_sparse_backtracks" and "tfm_sparse_l0"
 * (the L the first iteration began with: lipschitz, or the power estimate) of the last call.
 * "tfm_chunk" and the "tfm_model_*" options apply as in alifmm_tfm_lsq (with more than one slab what A
 * writes is zeroed every time).  One GPU. */
int alifmm_tfm_sparse(alifmm_ctx* ctx, int subgrid, int ntx, const int32_t* tx_slot, int nrx, const int32_t* rx_slot,
                      const double* fmc, int nt, int ncomp, double t0, double fs, const float* pair_w, int iz0, int ix0,
                      int niz, int nix, int step, double damp, double smooth, int max_iter, double tol, int ntap,
                      int tap_comp, const double* taps, int origin, double lam, double lipschitz, int power_iters,
                      int restart, double* image, double* resid, double* info12);

/* Travel-time sensitivities along rays: for every ray, the derivative of its time of flight in
 * every coarse cell it crosses (Fermat: to first order the path is fixed) — the rows of the
 * travel-time tomography Jacobian, and / or their weighted sums over the rays as three maps on the
 * coarse grid (with residuals as weights: the misfit gradient J^T r, beside a coverage map).  The
 * reference carries the pieces (slown_d_slown_stif :3468, travel_times :3026) but never uses them.
 *   subgrid            the points' subgrid
 *   ray_len[nrays]     points per ray
 *   flags (nullable)   the flags of alifmm_find_rays
 *   ray_xy (nullable)  packed points on the fine grid of `subgrid`, in the layout of
 *                      alifmm_find_rays (ray k's x at ray_xy[2*off[k] + 2*i], z at +1, off[k] = sum
 *                      of ray_len[0..k-1]); uploaded in chunks into grow-only buffers of the context.
 *                      NULL: the points kept on the device by the last alifmm_find_rays(..., NULL,
 *                      ALIFMM_KEEP_RAYS), read in place; they stay kept for alifmm_take_rays.  Only
 *                      the device-resident keep (one subgrid in that call, which the caller passes
 *                      here) is supported: ALIFMM_E_ARG for points staged on the host (several
 *                      subgrids in one call), and unless ray_len adds up to the kept count
 *   ray_w (nullable)   float64 [nrays] weights of the maps (1)
 *   maps (nullable)    float64 [3][nnz][nnx]: sum_k w_k len, sum_k w_k time, sum_k w_k dth per cell
 *   row_ptr (nullable) int64 [nrays + 1]: the entries of ray k are row_ptr[k] .. row_ptr[k+1] - 1
 *   cap, col (int32), len, time, dth (float64), each [cap], each nullable: the entries (CSR)
 *   ray_status (nullable) int32 [nrays]: 1 for an invalid ray (below), else 0
 * A ray is its points; segment i joins points i and i + 1 and is walked exactly as
 * time_between_points() (:2835-2989) walks it, piece by piece (a piece ends where the segment
 * crosses a half-integer cell edge).  Every piece yields one entry, in walk order, segments in
 * order; entries are neither merged nor sorted (a cell may occur more than once in a row):
 *   col   y_pos * nnx + x_pos, the piece's coarse cell (the rounded midpoint, a negative index
 *         wrapped once as numba wraps it)
 *   len   piece_dist [m]
 *   time  len * s [s], s = 1 / group_vel_cell(cell, eff), eff = pymod(veln - angle, 180): the very
 *         summand of time_between_points(); the ordered sum of a ray's time entries is its time
 *   dth   len * ds [s per degree of the cell's veln]
 * ds: with h = 2^-10 degree and s(e) = 1 / group_vel_cell(cell, e),
 *   ds = (s(pymod(eff + h, 180)) - s(pymod(eff - h, 180))) * 512,
 * except ds = 0 for a Christoffel cell (velpn == 0 with a stiffness row) inside the reference's
 * on-axis snap (eff % 90 < 0.01 or > 89.99), as slown_d_slown_stif returns there.  One rule for
 * every material kind: on a table material it is the table's slope, except within h of a knot.  h
 * is part of the contract: truncation (~ h^2 / 6 s''') and rounding (~ 2^-53 s / h) both come to
 * ~1e-9 of a typical derivative there.  dth inherits the snap's tiny discontinuity next to the axes
 * (within h of the snap one of the two slownesses is the snapped one).  The derivative in the
 * velocity scale needs no output of its own: d t / d vel_map[c] = - time_c / vel_map[c].
 * A ray contributes nothing (no entries, nothing in the maps) when flags[k] has bit 1 or bit 2 set
 * (the rays alifmm_find_rays cut short and never times), when ray_len[k] < 2, or when it is
 * invalid, ray_status[k] = 1: a coordinate is not finite, a piece's cell lies outside the grid after
 * the wrap, or a segment is unfinished after B = floor|x2 - x1| + floor|y2 - y1| + 4 pieces
 * (coordinates after the division by subgrid).  No finite walk needs more than B pieces, and the
 * bound is what ends the call on any input: a horizontal segment at z = k + 0.5, k odd, never sets
 * fin_y in time_between_points() (a vertical one at x = k + 0.5 never fin_x) and would walk off the
 * grid without end.
 * The rows are bit-reproducible, and a ray's rows depend neither on its place in the request nor
 * on its neighbours.  The maps are accumulated with float64 atomic adds, in no fixed order: they are
 * reproducible to rounding only, not bit for bit (a ray of weight 0 adds nothing).
 * Sizing: row_ptr alone (no row array) runs the count pass only; with a row array cap must be >=
 * row_ptr[nrays], else ALIFMM_E_ARG, row_ptr still holding the sizes.  All offsets are 64-bit.
 * ALIFMM_E_ARG with a message, the context staying usable, also when: the context has no model;
 * subgrid < 1; nrays < 0; ray_len is NULL; nothing is requested (maps, row_ptr and ray_status NULL);
 * a row array without row_ptr.  One GPU: maps of rays traced on several GPUs add on the host.
 * alifmm_get_option: "sens_upload_ms" (host -> device copies), "sens_kernel_ms" (count and fill
 * kernels) and "sens_entries" (row_ptr[nrays]) of the last call. */
int alifmm_ray_sens(alifmm_ctx* ctx, int subgrid, int nrays, const int32_t* ray_len, const int32_t* flags,
                    const double* ray_xy, const double* ray_w, double* maps, int64_t* row_ptr, int64_t cap,
                    int32_t* col, double* len, double* time, double* dth, int32_t* ray_status);

/* The inversion step on the device: one quantity of the rays' Jacobian kept in the context as an
 * operator A (nrays x ncell, ncell = nnz * nnx), products with it in both directions, and the
 * damped, smoothed least-squares step min |A x - rhs|^2 + damp^2 |x|^2 + smooth^2 |D x|^2 by CGLS.
 * One coarse-grid map comes back instead of the rows.
 *
 * alifmm_sens_op_build
 *   subgrid, nrays, ray_len, flags, ray_xy   the request, exactly as in alifmm_ray_sens (ray_xy NULL:
 *                      the points kept by the last alifmm_find_rays(..., NULL, ALIFMM_KEEP_RAYS))
 *   quantity           0 len, 1 time, 2 dth: which value of an entry the operator holds
 *   col_scale (nullable) float64 [ncell] cs (1): cs[c] == 0 freezes cell c; cs = -1 / vel_map with
 *                      quantity 1 gives the Jacobian in the velocity scale
 *   entries (nullable) the operator's entries = "sens_entries" of alifmm_ray_sens for the request
 *   ray_status (nullable) int32 [nrays], as alifmm_ray_sens
 * A[k][c] = cs[c] * (the sum of val[e] over the entries e of ray k with col[e] == c), the entries
 * being those of alifmm_ray_sens for the same request: the same walk, the same len / time / dth
 * arithmetic, the same kernels.  A skipped ray (flags bit 1 or 2, fewer than 2 points) and an invalid
 * one (ray_status 1) are empty rows.  Rows stay unmerged: a cell may occur several times in a row.
 * The context keeps the rows (CSR: row_ptr, col, val) and a transposed copy (CSC: col_ptr, row,
 * val) in which every column holds its entries in ascending entry index, that is by ray, then in
 * walk order (a stable sort by column): the order is a function of the request alone.  About 24
 * bytes per entry; fewer than 2^31 entries, else ALIFMM_E_CAPACITY.  A build replaces the resident
 * operator (a build refused with ALIFMM_E_ARG leaves it in place).  The operator is freed by alifmm_sens_op_release, with the context, and by
 * alifmm_set_model: it belongs to the model it was built on, and after a new model apply and solve
 * return ALIFMM_E_ARG until the next build.
 *
 * alifmm_sens_op_apply    out[nrays] = A in[ncell], or with transpose != 0 out[ncell] = A^T in[nrays]
 * (host vectors).  Term by term, in float64, no contraction:
 *   (A x)[k]   = sum over the entries e of row k, of val[e] * (cs[col[e]] * x[col[e]]); an empty row: 0
 *   (A^T y)[c] = cs[c] * (sum over the entries e of column c, of val[e] * y[row[e]]); an empty column: 0
 * Every sum has an order fixed by the operator: 256 lanes take a row's entries round robin, each adds
 * its own in order from 0, the 64 lanes of a wavefront pair up over the lane distances 32, 16, ..., 1,
 * the four wavefronts as (0 + 1) + (2 + 3); a column of up to 4 entries is added in order by one lane,
 * of up to 256 by the 64 lanes of one wavefront, a longer one as a row.  There are no float atomics:
 * two calls, two builds of the same request and two contexts return the same bits, and a ray's
 * element of A x depends on that ray alone.
 *
 * alifmm_sens_op_solve    CGLS from x = 0; D is the first difference over every 4-neighbour pair of
 * coarse cells that both have cs != 0, so (D^T D p)[c] = sum over those neighbours c' of
 * (p[c] - p[c']) (upper, left, right, lower, in that order; 0 in a frozen cell).  With
 * R(v) = damp^2 v + smooth^2 D^T D v:
 *   r = rhs; s = A^T r; p = s; gamma_0 = gamma = |s|^2; gamma_0 == 0: stop (breakdown)
 *   iteration it = 1, 2, ...:
 *     q = A p; qq = |q|^2 + p . R(p); qq == 0: stop (breakdown; the iteration does not count)
 *     alpha = gamma / qq; x += alpha p; r -= alpha q
 *     s = A^T r - R(x); gamma' = |s|^2; beta = gamma' / gamma; p = s + beta p; gamma = gamma'
 *     gamma <= tol^2 gamma_0: stop (tol); it == max_iter: stop (max_iter)
 * No augmented residual is kept.  All vectors and alpha, beta, gamma stay on the device; the host
 * reads 8 bytes per iteration for the stop rule.  Every dot product is a two-stage sum in a fixed
 * order (its partial sums depend on the vector's length alone), so x and info8 are bit-reproducible.
 * A frozen cell of x is exactly 0.
 *   rhs   float64 [nrays]; x float64 [ncell]
 *   info8 (nullable) iterations, sqrt(gamma_0), sqrt(gamma) at the end, |rhs|, the recurred |r| at the
 *         end, the stop's reason (0 tol, 1 max_iter, 2 breakdown), the operator's entries, 0
 *
 * ALIFMM_E_ARG with a message, the context staying usable, when: the context has no model; build:
 * subgrid < 1, nrays < 0, ray_len NULL, the kept-points errors of alifmm_ray_sens, quantity outside
 * 0..2, a col_scale that is not finite; apply and solve: no resident operator (never built, released,
 * or dropped by alifmm_set_model), in, out, rhs or x NULL, an rhs that is not finite, damp or smooth
 * negative or not finite, max_iter < 1, tol negative or not finite.  A failed device allocation
 * returns ALIFMM_E_HIP with the operator released.  One GPU.
 * alifmm_get_option: "solve_build_ms" (the last build, the whole call), "solve_kernel_ms" (device time
 * of the last apply or solve), "solve_iters" (the last solve) and "sens_op_entries" (the resident
 * operator's entries, 0 without one). */
int alifmm_sens_op_build(alifmm_ctx* ctx, int subgrid, int nrays, const int32_t* ray_len, const int32_t* flags,
                         const double* ray_xy, int quantity, const double* col_scale, int64_t* entries,
                         int32_t* ray_status);
int alifmm_sens_op_apply(alifmm_ctx* ctx, int transpose, const double* in, double* out);
int alifmm_sens_op_solve(alifmm_ctx* ctx, const double* rhs, double damp, double smooth, int max_iter, double tol,
                         double* x, double* info8);
int alifmm_sens_op_release(alifmm_ctx* ctx);

/* n straight-segment times on the resident model (time_between_points() :2835-2989; the
 * coordinates are fine-grid indices of `subgrid`).  ray_time() (:2992-3022) = ordered sum. */
int alifmm_time_between_points(alifmm_ctx* ctx, int n, const double* x1, const double* x2, const double* y1,
                               const double* y2, int subgrid, double* out);

/* Evaluate the local operators on n independent neighbourhoods (pz x px patches; rows past pz
 * read as nsts=-1/ttn=0, the reference's padded stage-1 semantics).  op 0: update() :904-1410
 * with the phase table; op 1: fouds18_A() :240-901 with the group table.  Material is given at
 * the target cell only (the operators read nothing else); cell_stif (n x 5) NULL = None.
 *
 * Ops 3, 4 and 5 are test entry points: the same inputs through the forms of the operators that
 * the field kernels run, each held to the bits of ops 0 / 1 (tests/test_gpu_local_ops.py).
 *   3  update() on a register neighbourhood: the patch coded as the device grids are (NaN where
 *      nsts < 0), read by the kernels' 12-point loader with its clamped addresses, then the
 *      branch-free selection under update()'s bounds (nnz_arg / nnx_arg).
 *   4  as 3 with the selection spread over one wavefront per case (the exact walks' relax step).
 *   5  fouds18_A() on four lanes per case, one candidate of each stencil family per lane,
 *      reduced and combined as in the band kernel's fallback rounds.
 * (2 and 6 are alifmm_fouds18_band and alifmm_fouds18_band_lanes.)  The kernels' own lane-local
 * slot loaders from LDS are private to them and are not reached from here.
 * ALIFMM_E_ARG: any other op; for ops 3..5 also a cell outside its patch, an nnx_arg above px, or
 * a ttn that is not finite at a node with nsts >= 0.  The context stays usable. */
int alifmm_local_ops(alifmm_ctx* ctx, int op, int n, int pz, int px, const double* ttn, const int32_t* nsts,
                     const int32_t* iz, const int32_t* ix, const double* dnx, const double* dnz,
                     const int32_t* nnz_arg, const int32_t* nnx_arg, const double* cell_veln,
                     const int64_t* cell_velpn, const double* cell_vm, const int64_t* cell_stif,
                     const double* tab, int ncol, double* out);

/* Evaluate the correctly rounded trigonometric functions every operator calls (csrc/cr_math.h) on
 * n arguments, one per device thread: a device-level parity test like alifmm_local_ops.  fn 0 atan,
 * 1 sin, 2 cos, 3 tan: out[i] = f(x[i]); fn 4 sincos: out[i] = sin, out2[i] = cos (out2 is required
 * for fn 4 and ignored otherwise).  lds_tables 0: the kernel reads the functions' tables from global
 * constants; 1: from LDS after crm::lds_init(), as the solver and ray kernels do.  n = 0 succeeds and
 * launches nothing.  ALIFMM_E_ARG, with out / out2 untouched: fn or lds_tables out of range, n < 0,
 * a null x / out (/ out2 for fn 4) with n > 0. */
int alifmm_cr_math(alifmm_ctx* ctx, int fn, int lds_tables, int64_t n, const double* x, double* out, double* out2);

/* fouds18_A() (:240-901) exactly as the band kernel evaluates it: the material of resident-model
 * cell (mz, mx) through the model's per-material record and its precomputed stencil slownesses
 * (quant 1: the subgrid > 1 view, orientation truncated to int32 and vel_map to float32, as
 * finer_grid_n does at :26-56).  Same patches and arguments as alifmm_local_ops op 1. */
int alifmm_fouds18_band(alifmm_ctx* ctx, int n, int pz, int px, const double* ttn, const int32_t* nsts,
                        const int32_t* iz, const int32_t* ix, const double* dnx, const double* dnz,
                        const int32_t* nnz_arg, const int32_t* nnx_arg, const int32_t* mz, const int32_t* mx,
                        int quant, double* out);

/* Test entry point (op 6): alifmm_fouds18_band on four lanes per case, the candidates split and
 * reduced as in the band kernel's fallback rounds.  Same arguments, same bits; the argument
 * checks of alifmm_local_ops ops 3..5 on top of alifmm_fouds18_band's (ALIFMM_E_ARG: no model). */
int alifmm_fouds18_band_lanes(alifmm_ctx* ctx, int n, int pz, int px, const double* ttn, const int32_t* nsts,
                              const int32_t* iz, const int32_t* ix, const double* dnx, const double* dnz,
                              const int32_t* nnz_arg, const int32_t* nnx_arg, const int32_t* mz,
                              const int32_t* mx, int quant, double* out);

/* ---- RCCL gather of resident fields onto one GPU (replaces the reference's result return over
 * multiprocessing queue2: parallel_TTF :3610, parallel_TTF_finer_grid :3659, parallel_TTF_rays
 * :3733).  librccl is loaded on first use.  A communicator spans one GPU per rank:
 *   alifmm_comm_init_all   one process driving n contexts on n distinct GPUs (ranks = array order)
 *   alifmm_comm_init_rank  one process per GPU; every rank passes the same 128-byte id, made by one
 *                          rank with alifmm_comm_unique_id and shared by the caller's own means. */
typedef struct alifmm_comm alifmm_comm;
int alifmm_comm_unique_id(char* id128);
int alifmm_comm_init_rank(alifmm_ctx* ctx, int nranks, int rank, const char* id128, alifmm_comm** out);
int alifmm_comm_init_all(alifmm_ctx* const* ctxs, int n, alifmm_comm** out);
int alifmm_comm_destroy(alifmm_comm* comm);
const char* alifmm_comm_last_error(alifmm_comm* comm);
/* Every rank calls it with the same arrays (indexed by rank): rank r's resident slots
 * first_slot[r] .. first_slot[r]+count[r]-1 (fields of `subgrid`, one shape) arrive on the root as
 * resident slots dst_slot + count[0] + ... + count[r-1] + i, rank after rank (one ncclSend /
 * ncclRecv per field in one group; no padding).  The root's own fields stay in place when their
 * destination equals their slots, else they are copied device-to-device into free slots.
 * *ms (nullable) = wall time of the gather on this process. */
int alifmm_gather_fields(alifmm_comm* comm, int root, int subgrid, const int* first_slot, const int* count,
                         int dst_slot, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* ALIFMM_H */
