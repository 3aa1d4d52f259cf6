// nr_k6_tune.h -- the shape knobs of K6's band kernels in one place.
//
// The product build takes the defaults below.  Development builds (neural_renderer_amd._build.build_variant, timed side
// by side through NR_HIP_LIB) override single numbers with -D...  Besides these, only the two measurement builds are
// conditional on macros: NR_PROFILE_HOOK (the band kernel's timing hook) and NR_ROW_STATS (k_bpm_row's work counters).
// k_bpm_fast's tolerance-mode arithmetic has no switches: fused multiply-adds for diff and dist, one v_rcp_f32 per term, float
// piece and run sums.  Round 4 measured the alternatives (profiles/r04_k6_numerics.jsonl, LAB-NOTEBOOK): no accumulation knob
// moved the default mode's error level.
#pragma once

#ifndef NR_K6_FB           // pixels of an unrolled piece whose LDS reads are requested together (FSEG is a multiple;
#define NR_K6_FB 3         // 1 / 3 / 5 -> stage 229 / 230 / 252 us, 3 needs the fewest registers)
#endif
#ifndef NR_K6_U_GROUP      // class U pieces per super-piece (one descriptor / decode / flush for up to this many pieces of 15 pixels;
#define NR_K6_U_GROUP 3      // 1: every piece on its own, rounds 3-4; at most 4: the count travels in two bits)
#endif
#ifndef NR_K6_SMALL_RASTER_MAX  // up to this raster size: 256-thread workgroups on two-line bands (band_shape; 0: never)
#define NR_K6_SMALL_RASTER_MAX 400
#endif
#ifndef NR_K6_MINWAVES_256  // launch bound (waves per SIMD) of the 256-thread shape
#define NR_K6_MINWAVES_256 4
#endif
#ifndef NR_K6_WMAX         // widest band (lines per workgroup) of the 512-thread shape
#define NR_K6_WMAX 4
#endif
#ifndef NR_K6_FOLD_KB      // largest slice of the fused backward's grad_textures fill that a band workgroup takes along
#define NR_K6_FOLD_KB 128
#endif
#ifndef NR_K6_LDS_BUDGET   // (512-thread shape) three workgroups per 160 KB CU, allocation granules of 512 bytes included (3 x 53.5 KB would not fit)
#define NR_K6_LDS_BUDGET (53 * 1024)
#endif

#ifndef NR_K6_WIDE_BUDGET_FROM  // rasters in (FROM, TO]: the 512-thread shape with 80 KB of LDS per workgroup (band_shape)
#define NR_K6_WIDE_BUDGET_FROM 576
#endif
#ifndef NR_K6_WIDE_BUDGET_TO
#define NR_K6_WIDE_BUDGET_TO 832
#endif
#ifndef NR_K6_OVF_GRID      // workgroups of k_bpm_fast's overflow-only launch behind k_bpm_row (images whose records exceed the line buffer):
#define NR_K6_OVF_GRID 256  // one per CU -- a launch whose workgroups leave at once costs 1.3 us up to 256 of them, 1.6 at 1024, 2.3 at
#endif                      // 4096, 4.6 at 16 384 (scripts/dev/empty_launch_probe.hip); fused backward at the headline shape 214.4 -> 212.5 us
#ifndef NR_ROW_MIN_WGS      // k_bpm_row: four-line bands become two-line bands while the launch has fewer band workgroups than this ...
#define NR_ROW_MIN_WGS 4096
#endif
#ifndef NR_ROW_MIN_WGS_1    // ... and two-line bands one-line bands below this many
#define NR_ROW_MIN_WGS_1 1024
#endif

#ifndef NR_SHARED_LAUNCH_MAX_FACES  // fused backward: calls of up to this many faces (batch x faces) put the line setup and the
#define NR_SHARED_LAUNCH_MAX_FACES 98304  // K7 / K8 gather into one launch (plan_backward; measured: LAB-NOTEBOOK, late round 4)
#endif
#ifndef NR_TAIL_GATHER_MAX_FACES  // fused backward: calls above NR_SHARED_LAUNCH_MAX_FACES and up to this many faces run the K7 / K8
#define NR_TAIL_GATHER_MAX_FACES 655360  // gather's workgroups behind k_bpm_row's in one grid (k_band_gather, plan_backward; 0: never).
#endif                                   // Fused backward, us, merged launch / serial order (teapot views, texture_size 2, all three
                                         // outputs; medians of 7 x 30 calls): 32 views at 256^2 117.3 / 138.9, 64 views 197.2 / 215.0,
                                         // 80 views 245.9 / 260.4, 96 views 285.5 / 300.8, 128 views (630 784 faces) 374.3 / 386.0,
                                         // 64 views at 512^2 606.9 / 620.0 -- and beyond the bound 256 views at 128^2 (1.26 M faces)
                                         // 333.0 / 324.7, 1024 views at 32^2 (5 M) 545.3 / 452.6: there the band kernel is short, the
                                         // gather's grid of F / 16 workgroups per image (most of which only read their list's length)
                                         // is long, and the fill inside the band kernel and the finish inside the gather are worth more.
                                         // Configs 4 and 5 (texture sizes 4 and 8) have no static-tap gather: serial order as before.
// The fused backward without its idle workgroups (profiles/idle_workgroups_ab.md; fused backward, us per call, medians of 7 rounds
// of 30 calls, the builds alternating in one process; teapot views at 256^2 unless said otherwise):
#ifndef NR_SLOT_STRIDE      // k_line_setup (alone or inside k_setup_gather) and the gather part of k_band_gather: a launch has ceil(slots /
#define NR_SLOT_STRIDE 4    // this) workgroups per image, each looping over slots that far apart while the image's list lasts (1: a
#endif                      // workgroup per slot).  A teapot view lists 19 % of its faces: at 4 almost no workgroup loops and three in four
                            // of those that only read their list's length and leave are not dispatched.  1 / 2 / 4 / 8: 64 views 178.8 /
                            // 179.3 / 178.8 / 179.2 (working-first order had taken it all there), 16 views 80.4 / 79.7 / 79.1 / 80.6,
                            // 8 views 60.7 / 60.7 / 59.9 / 65.1, 32 views 111.3 / 110.9 / 110.9 / 116.8, 1024 views at 32^2 457.8 /
                            // 437.7 / 428.6 / 425.0 -- at 8 the working workgroups of a view loop and the launch has a second round
#ifndef NR_MERGE_OVERFLOW   // 1: the overflow pass behind k_bpm_row rides in k_backward_big's launch where the plan finishes K6 there
#define NR_MERGE_OVERFLOW 1 // (k_big_overflow, nr_backward_pixel_map.hip); 0: a launch of its own, always.  0 / 1: 64 views 180.0 / 178.8,
#endif                      // 16 views 80.5 / 79.1, 8 views 61.6 / 59.9 (back to back the empty launch cost 1.2 ... 1.7 us, not the 4.6 of its trace)
#ifndef NR_SETUP_GATHER_IMAGE_FASTEST    // k_setup_gather's ids: 1 image fastest (working workgroups first, as k_line_setup's), 0 the
#define NR_SETUP_GATHER_IMAGE_FASTEST 1  // 2-D grid's order.  0 / 1: 16 views 84.5 / 79.1, 8 views 65.0 / 59.9
#endif
#ifndef NR_ROW_DEAL_IMAGES    // k_band_gather's band part: 1 the images dealt across the XCDs (batches of 16, 24, ...), 0 eight runs of
#define NR_ROW_DEAL_IMAGES 1  // neighbouring images (bpm_row_body).  0 / 1: 64 views 179.0 / 175.3, 32 views 110.7 / 108.0, 128 views
#endif                        // 344.9 / 333.3, 64 views at 512^2 575.5 / 572.0

namespace nr {
namespace k6 {
constexpr bool ROW_DEAL_IMAGES = NR_ROW_DEAL_IMAGES != 0;
constexpr unsigned SLOT_STRIDE = NR_SLOT_STRIDE;
static_assert(SLOT_STRIDE >= 1, "slots per workgroup of the strided launches");
constexpr bool MERGE_OVERFLOW = NR_MERGE_OVERFLOW != 0;
constexpr int FB = NR_K6_FB;
constexpr int U_GROUP = NR_K6_U_GROUP;
static_assert(U_GROUP >= 1 && U_GROUP <= 4, "a super-piece's count travels in two bits");
constexpr int SMALL_RASTER_MAX = NR_K6_SMALL_RASTER_MAX;
constexpr int MINWAVES_256 = NR_K6_MINWAVES_256;
constexpr int WMAX = NR_K6_WMAX;
constexpr int FOLD_KB = NR_K6_FOLD_KB;
constexpr unsigned long LDS_BUDGET = NR_K6_LDS_BUDGET;
constexpr unsigned long ROW_MIN_WGS = NR_ROW_MIN_WGS, ROW_MIN_WGS_1 = NR_ROW_MIN_WGS_1;
constexpr unsigned OVF_GRID = NR_K6_OVF_GRID;
constexpr int WIDE_BUDGET_FROM = NR_K6_WIDE_BUDGET_FROM, WIDE_BUDGET_TO = NR_K6_WIDE_BUDGET_TO;
constexpr unsigned long SHARED_LAUNCH_MAX_FACES = NR_SHARED_LAUNCH_MAX_FACES;
constexpr unsigned long TAIL_GATHER_MAX_FACES = NR_TAIL_GATHER_MAX_FACES;
}  // namespace k6
}  // namespace nr
