/*
 * fishbird.h -- C ABI of the MI355X-native front-end + optimiser path.
 *
 * This header is the drop-in boundary: every entry point names the reference
 * interface it replaces (file:line in JingruiYu/FishBirdEyeVisualSLAM).  Plain
 * pointers and sizes only; no C++/torch/OpenCV types.  INTEGRATION.md shows the
 * shim a maintainer adds inside ORBextractor / ORBmatcher / Optimizer.
 *
 * Pointer convention
 *   *_dev entry points take DEVICE pointers (HBM resident) and a hipStream_t
 *   passed as void*; they enqueue work and return without synchronising.
 *   Entry points without the suffix take HOST pointers, copy, run the same
 *   kernels and synchronise before returning (drop-in for the reference call).
 *   A host drop-in synchronises the stream it ran on, not the whole device; a
 *   null required array is FB_ERR_ARG, reported before anything is enqueued.
 *
 * Threads
 *   Calls that take no handle (matchers, pose optimisation, bundle adjustment)
 *   may run concurrently from several host threads, each on the device that is
 *   current for its thread.  A handle (fb_orb, fb_rccl communicator) carries
 *   device buffers of its own: one call at a time per handle, like the
 *   reference's ORBextractor object.  fb_last_error() is per thread.
 *
 * Status: 0 = ok, <0 = error (fb_last_error() gives the text).
 * There is no CPU fallback: without a HIP device every compute call fails with
 * FB_ERR_NODEVICE.
 */
#ifndef FISHBIRD_H_
#define FISHBIRD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FB_ABI_VERSION 1
#define FB_MAX_LEVELS 16
#define FB_DESC_BYTES 32 /* 256-bit rBRIEF, ORBextractor.cc:1068 */

enum {
  FB_OK = 0,
  FB_ERR_ARG = -1,      /* bad argument */
  FB_ERR_HIP = -2,      /* HIP runtime error */
  FB_ERR_CAPACITY = -3, /* an internal/declared capacity was exceeded */
  FB_ERR_NODEVICE = -4  /* no HIP device / kernels not loadable */
};

/* ---- runtime ------------------------------------------------------------ */
int fb_abi_version(void);
const char *fb_last_error(void);
int fb_device_count(void);
int fb_set_device(int device);
/* Releases what the library keeps between calls: the idle blocks of the device scratch pool (all devices) and the calling
 * thread's bundle-adjustment stream / event / pinned control block.  Handles (fb_orb, fb_frame, communicators) stay valid;
 * the next call simply allocates again.  Call it from every thread that ran a bundle adjustment before the thread ends. */
int fb_shutdown(void);

/* ---- per-kernel timing (HIP events on the launch stream) ------------------- */
/* When enabled every kernel launch of this library is bracketed by two hipEvents
 * recorded on the stream it is launched on; fb_prof_report synchronises and
 * returns launches and total milliseconds per kernel since fb_prof_reset.      */
typedef struct fb_prof_entry {
  char name[32];
  int32_t launches;
  double total_ms;
} fb_prof_entry;
int fb_prof_enable(int on);
int fb_prof_only(const char *kernel_name); /* bracket only this kernel (e.g. "k_fast"); NULL or "" = every kernel */
int fb_prof_reset(void);
int fb_prof_report(fb_prof_entry *out, int cap); /* returns the number of entries written */

/* cv::KeyPoint as POD (ORBextractor.cc:837-847: pt, size, angle, response, octave) */
typedef struct fb_keypoint {
  float x, y;
  float size;
  float angle;
  float response;
  int32_t octave;
} fb_keypoint;

/* ======================================================================== */
/* ORBextractor  (include/ORBextractor.h:51-85, src/ORBextractor.cc:410-1132) */
/* ======================================================================== */
typedef struct fb_orb fb_orb;

typedef struct fb_orb_params { /* ctor args, ORBextractor.h:51-52 */
  int32_t nfeatures;
  float scale_factor;
  int32_t nlevels;
  int32_t ini_th_fast;
  int32_t min_th_fast;
} fb_orb_params;

typedef struct fb_orb_tables { /* getters ORBextractor.h:63-83 + mnFeaturesPerLevel, umax */
  float scale_factor[FB_MAX_LEVELS];
  float inv_scale_factor[FB_MAX_LEVELS];
  float level_sigma2[FB_MAX_LEVELS];
  float inv_level_sigma2[FB_MAX_LEVELS];
  int32_t features_per_level[FB_MAX_LEVELS];
  int32_t umax[16];
} fb_orb_tables;

/* replaces ORBextractor::ORBextractor (ORBextractor.cc:410-470) */
int fb_orb_create(const fb_orb_params *params, fb_orb **out);
void fb_orb_destroy(fb_orb *h);
int fb_orb_get_tables(const fb_orb *h, fb_orb_tables *out);
/* Output capacity per image.  DistributeOctTree stops at >= N nodes, so a level can
 * return up to N+2 keypoints (ORBextractor.cc:669,729): capacity = nfeatures + 8*nlevels. */
int fb_orb_capacity(const fb_orb_params *params);
/* Entries per image in the output arrays of fb_orb_extract_batch_dev when the caller's arrays are wider than the
 * capacity (an fb_frame shares one stride between a 2000-feature front and a 1000-feature bird extractor).  0 = capacity. */
int fb_orb_set_output_stride(fb_orb *h, int kp_stride);

/* replaces ORBextractor::operator() (ORBextractor.cc:1043-1105), host buffers.
 * image: u8, row-major, `stride` bytes per row.  keypoints/descriptors must hold
 * cap = fb_orb_capacity() entries (desc: cap*32 bytes).  *n_out <= cap.
 * cap = nfeatures + 8*nlevels covers the quadtree's overshoot of at most 3 per level; a level can also end with up
 * to 4x its number of root nodes (a strip many times wider than high with a tiny feature budget): if that exceeds cap,
 * FB_ERR_CAPACITY is returned.                                                  */
int fb_orb_extract(fb_orb *h, const uint8_t *image, int width, int height, int stride,
                   fb_keypoint *keypoints, uint8_t *descriptors, int32_t *n_out);

/* same, `batch` equally sized images resident in HBM; image b starts at
 * d_images + b*image_stride.  Outputs: d_keypoints[batch][cap],
 * d_descriptors[batch][cap][32], d_n[batch], cap = fb_orb_capacity(); d_n[b] is
 * clamped to cap (asynchronous call: no error channel for the overflow above).
 * Stream semantics: everything is ordered after the work already in `stream` and is complete for work enqueued to
 * `stream` afterwards.  By default every kernel runs on `stream`.  Only when the environment variable FB_ORB_SIDE_MIN is
 * set do calls of at least that many images run the Gaussian blur on a stream the handle owns, forked from and joined
 * back into `stream` with events inside the call (legal under stream capture as well).
 * The first call at a new image size, or with a larger batch, sizes the handle's workspace (it allocates, so it is not
 * for stream capture).  A call that returns an error, a refused image size included, leaves the handle usable at its
 * previous size: the next call at that size runs as if the failed one had not been made.  */
int fb_orb_extract_batch_dev(fb_orb *h, const uint8_t *d_images, int batch, int width, int height,
                             int stride, size_t image_stride, fb_keypoint *d_keypoints,
                             uint8_t *d_descriptors, int32_t *d_n, void *stream);

/* ORB descriptors at key points the CALLER supplies: ORBextractor::computeDescriptors on a given list, cv::ORB::compute of
 * OpenCV 3 (features2d/src/orb.cpp), restated.  Frame.cc:352-355 calls it on the bird key points after cv::cornerSubPix has
 * moved them.  The call works on the pyramid and the blurred pyramid the handle holds from its LAST extract call (images
 * b < batch of that call), and returns FB_ERR_ARG when nothing has been extracted yet, when `batch` exceeds that call's
 * batch, or when FB_DESCRIBE_IC_ANGLE is asked for without `images`.  For key point i < min(n[b], kp_stride) of image b:
 *   level     l = octave.  l < 0 or l >= nlevels: status FB_DESCRIBE_LEVEL, nothing of the key point is written.
 *   position  px = cvRound(x * inv_scale_factor[l]), py = cvRound(y * inv_scale_factor[l]): the product in float, rounded
 *             to nearest with halves to even (OpenCV 3: cvRound(kpt.pt.x * scale), scale = 1 / getScale(octave)).
 *   border    unless 19 <= px <= w_l - 20 and 19 <= py <= h_l - 20 (EDGE_THRESHOLD: the range in which the extractor
 *             itself places key points, so that neither patch leaves the level): status FB_DESCRIBE_BORDER, the descriptor
 *             row and the angle stay as they were.  The test is made on the rounded float before it becomes an integer:
 *             NaN and +-inf coordinates are FB_DESCRIBE_BORDER.
 *   angle     FB_DESCRIBE_KEEP_ANGLE: kps[i].angle as given (degrees; OpenCV 3 does not re-orient supplied key points).
 *             It is expected to be finite; a non-finite angle gives an unspecified descriptor and no out-of-range access.
 *             FB_DESCRIBE_IC_ANGLE: IC_Angle (ORBextractor.cc:77-104, cv::fastAtan2) on the RAW level l at (px, py),
 *             written to kps[i].angle.  Level 0 of the raw pyramid is the caller's image, which the handle never copies:
 *             `images`, `stride` and `image_stride` are those of the extract call (any alignment).
 *   desc      computeOrbDescriptor (ORBextractor.cc:107-147) on the BLURRED level l at (px, py) with that angle: 32 bytes,
 *             status FB_DESCRIBE_OK.
 * x, y, size, response, octave and every entry at or past n[b] are never written.
 * There is NO compaction: cv::ORB::compute erases the key points too close to the border (KeyPointsFilter::runByImageBorder)
 * and thereby shifts every index behind them; here the count and the indices stay -- arrays that run beside the key points
 * (map points, grid cells) keep their meaning -- and the caller reads the status byte instead.
 * kps, desc and n are 4-byte aligned (_dev).  One wave per key point: DESIGN.md section 4. */
enum { FB_DESCRIBE_OK = 0, FB_DESCRIBE_BORDER = 1, FB_DESCRIBE_LEVEL = 2 };
enum { FB_DESCRIBE_KEEP_ANGLE = 0, FB_DESCRIBE_IC_ANGLE = 1 };
typedef struct fb_orb_describe_args {
  int32_t batch, kp_stride;
  const int32_t *n;                     /* [batch]                                                               */
  fb_keypoint *kps;                     /* [batch][kp_stride]  only .angle is ever written, only in IC mode      */
  uint8_t *desc;                        /* [batch][kp_stride][32]                                                */
  uint8_t *status;                      /* optional [batch][kp_stride]  FB_DESCRIBE_*                            */
  int32_t angle_mode;                   /* FB_DESCRIBE_KEEP_ANGLE / FB_DESCRIBE_IC_ANGLE                         */
  const uint8_t *images;                /* the images of the extract call; needed for IC mode only               */
  int32_t stride;                       /* their bytes per row                                                   */
  size_t image_stride;                  /* image b starts b * image_stride bytes after `images`                  */
} fb_orb_describe_args;
int fb_orb_describe_dev(fb_orb *h, const fb_orb_describe_args *a, void *stream);  /* device pointers */
int fb_orb_describe(fb_orb *h, const fb_orb_describe_args *a);                    /* host pointers   */

/* cv::ORB's detector: cv::ORB::create(nfeatures)->detect(image, mask) of OpenCV 3 (features2d/src/orb.cpp computeKeyPoints,
 * HarrisResponses, ICAngles, KeyPointsFilter::retainBest / runByImageBorder / runByPixelsMask, and cv::FAST with
 * nonmaxSuppression), restated; OpenCV is not vendored, so parity with it is unpinned like cornerSubPix and
 * fb_orb_describe.  Frame.cc:337 calls it on the bird image.  nfeatures, nlevels and scale_factor are the handle's;
 * ini_th_fast and min_th_fast are unused.  Per image b and per level l of the handle's pyramid:
 *   pyramid   the handle's own raw levels (ORBextractor::ComputePyramid, the tables of fb_orb_get_tables).  cv::ORB sizes
 *             its levels with cvRound(cols / (float)pow(scaleFactor, l)) and scales pt and size by that power; here the
 *             sizes are cvRound(cols * inv_scale_factor[l]) and the scale is scale_factor[l].
 *   mask      optional, u8, `height` rows of `mask_stride` bytes, shared by the batch.  m_0 = mask; for l >= 1
 *             m_l = tozero_254(resize(m_{l-1})): the bilinear resize of the image levels applied to the already
 *             thresholded previous level, then a value is kept iff it is > 254 (THRESH_TOZERO at 254), else 0.  A
 *             candidate at integer (px, py) of level l survives iff m_l[py][px] != 0: at level 0 any nonzero value passes,
 *             above it only pixels that interpolate to exactly 255.  The mask levels are rebuilt on every call, in a buffer
 *             of the handle: like the pyramids they serve one caller at a time.
 *   FAST      FAST-9-16 at the one threshold `fast_threshold` on the pixels [3, w_l - 3) x [3, h_l - 3) of the whole level
 *             (a pixel outside counts as score 0), the corner test and cornerScore of the extractor; 3x3 non-maximum
 *             suppression, strictly greater than all 8 neighbours (two equal neighbours drop each other).
 *   border    kept iff 31 <= px < w_l - 31 and 31 <= py < h_l - 31; a level with w_l <= 62 or h_l <= 62 yields nothing.
 *   cut 1     K1 = 2 * features_per_level[l]: with more than K1 candidates, exactly those whose FAST score is >= the
 *             K1-th largest score stay -- ties at the cut all stay, so more than K1 may (retainBest).  K = 0 keeps none.
 *   Harris    integer sums a = sum Ix^2, b = sum Iy^2, c = sum Ix Iy of the 3x3 Sobel derivatives over the 7 x 7 block
 *             around (px, py); response = ((float)a*(float)b - (float)c*(float)c - k*((float)a+(float)b)*((float)a+(float)b))
 *             * s4, k = 0.04f, s = 1.f/(4*7*255.f), s4 = s*s*s*s, every float operation rounded on its own, left to right.
 *   cut 2     K2 = features_per_level[l], the same rule on the Harris response compared as floats (-0.0 equals 0.0).
 *   angle     IC_Angle on the raw level at (px, py) (what FB_DESCRIBE_IC_ANGLE computes).
 *   output    x = (float)px * scale_factor[l], y likewise, size = 31.f * scale_factor[l], angle, response = Harris,
 *             octave = l.  cvRound(x * inv_scale_factor[l]) == px, so fb_orb_describe lands on the detected pixel.
 *   order     levels ascending, raster order (py, then px) within a level.  (OpenCV's order after nth_element is
 *             implementation-defined: the SET is what is shared with it, the order is this library's choice.)
 *   capacity  kps holds kp_stride entries per image (fb_orb_capacity() is the recommended value).  Ties can make the
 *             total exceed it: the first kp_stride entries in output order are written, n[b] = kp_stride, and n_true[b]
 *             (optional) receives the untruncated total.  Entries at or past n[b] are never written.
 * The call builds the handle's raw and blurred pyramid as an extract call does and counts as the handle's last extraction:
 * fb_orb_detect followed by fb_orb_describe(FB_DESCRIBE_KEEP_ANGLE) is cv::ORB::detectAndCompute without the compaction.
 * Workspace and failure behaviour are those of fb_orb_extract_batch_dev (the first call at a size allocates; a refused call
 * leaves the handle as it was); a later extract call on the handle gives what it gave before.  batch = 0 is a no-op.
 * No host round trip and no synchronisation inside the _dev call.  kps, n and n_true are 4-byte aligned (_dev).
 * Kernels: DESIGN.md section 4.                                                                                          */
typedef struct fb_orb_detect_args {
  int32_t batch, width, height, stride; /* `batch` u8 images of width x height, `stride` bytes per row                   */
  size_t image_stride;                  /* image b starts b * image_stride bytes after `images`                          */
  const uint8_t *images;
  const uint8_t *mask;                  /* optional: one mask of `height` rows, `mask_stride` bytes apart, for the batch */
  int32_t mask_stride;
  int32_t fast_threshold;               /* cv::ORB default 20; 1..255                                                    */
  int32_t kp_stride;
  fb_keypoint *kps;                     /* [batch][kp_stride]                                                            */
  int32_t *n;                           /* [batch]                                                                       */
  int32_t *n_true;                      /* optional [batch]                                                              */
} fb_orb_detect_args;
int fb_orb_detect_dev(fb_orb *h, const fb_orb_detect_args *a, void *stream);  /* device pointers */
int fb_orb_detect(fb_orb *h, const fb_orb_detect_args *a);                    /* host pointers, through the Stager */
/* The same with one mask PER IMAGE: the mask of image b starts b * mask_image_stride bytes after a->mask (at least
 * mask_stride * height; 0 = one mask shared by the batch, which is fb_orb_detect_dev).  The handle then holds one mask
 * pyramid per image.  fb_frame_extract_dev uses it: a frame's detect masks are per image.                               */
int fb_orb_detect_masks_dev(fb_orb *h, const fb_orb_detect_args *a, size_t mask_image_stride, void *stream);

/* debug/parity access to the pyramid level of image `b` of the last batch
 * (public member mvImagePyramid, ORBextractor.h:85). dst is host, w*h bytes.  */
int fb_orb_get_level(fb_orb *h, int b, int level, uint8_t *dst, int *w, int *hgt);
/* debug/parity: the same level after GaussianBlur(7x7, 2, 2, BORDER_REFLECT_101) (ORBextractor.cc:1080),
 * the image computeDescriptors samples.  dst is host, w*h bytes of fb_orb_get_level's size. */
int fb_orb_get_blurred_level(fb_orb *h, int b, int level, uint8_t *dst);
/* debug/parity: FAST candidates of (image b, level) of the last batch, the input of
 * DistributeOctTree (vToDistributeKeys, ORBextractor.cc:822-824), packed
 * x | y<<12 | response<<24 in level coordinates, unordered.  Returns the count (>=0). */
int fb_orb_debug_candidates(fb_orb *h, int b, int level, uint32_t *dst, int cap);
/* debug/parity: which resize kernel built pyramid level `level` (1 .. nlevels-1) in the last call: 0 = k_resize (any
 * source), 1 = k_resize_rows, 2 = k_resize_merge (both need a source whose pointer, row stride and image stride are
 * multiples of 4 and level sizes that keep their windows).  Host state only; a negative value is an error code. */
int fb_orb_debug_resize_route(fb_orb *h, int level);
/* profiling aid: with FB_FAST_DBG=20 one k_fast workgroup in 16 accumulates shader-clock cycles per phase
 * (0 address set-up + load issue, 1 tile wait, 2 sweep, 3/4/5 score/NMS/slot reservation at iniThFAST, 6/7/8 the same
 * at minThFAST, 9 cell decode, 10 whole wave, 11 number of timed waves); reading resets the counters.          */
int fb_orb_debug_timers(fb_orb *h, uint64_t *dst16);

/* ======================================================================== */
/* Frame grid (src/Frame.cc:381-411, 548-570; include/Frame.h:38-40)         */
/* ======================================================================== */
typedef struct fb_grid_geom {
  float min_x, min_y;       /* mnMinX, mnMinY (0 for the bird grid)            */
  float inv_w, inv_h;       /* mfGridElementWidthInv / HeightInv               */
  int32_t cols, rows;       /* 64x48 front, 32x32 bird                         */
} fb_grid_geom;

/* AssignFeaturesToGrid (Frame.cc:381-411): CSR with cell id = ix*rows+iy, items
 * in ascending keypoint index.  d_cell_start[batch][cols*rows+1],
 * d_cell_items[batch][cap].  Keypoints are read at kp_stride entries per image. */
int fb_grid_build_batch_dev(const fb_keypoint *d_keypoints, const int32_t *d_n, int batch,
                            int kp_stride, const fb_grid_geom *geom, int32_t *d_cell_start,
                            int32_t *d_cell_items, void *stream);

/* Bird keypoint -> base XY -> camera XYZ (Frame.cc:365-373, Converter.cc:284-292,312-318):
 * d_cam_xyz[b][i] = Tcb * BirdPixel2BaseXY(kps[i]).  Tcb = rows 0..2 of Frame::Tcb. */
int fb_bird_keys_to_cam_dev(const fb_keypoint *d_kps, const int32_t *d_n, int batch, int kp_stride,
                            int bird_cols, int bird_rows, double pixel2meter,
                            double rear_axle_to_center, const float *Tcb12 /* host */,
                            float *d_cam_xyz, void *stream);

/* Frame::GuidenceKeyBirdPts + nearEdges + genEdgesPC (src/Frame.cc:671-739, called at :342 between the bird
 * detect and compute steps) and the mask of extractorBird->detect(img, kps, mask) (Frame.cc:337-339).
 *
 * A bird key point survives iff
 *   (mask == NULL || mask[(int)(y + .5f)][(int)(x + .5f)] != 0)          -- cv::KeyPointsFilter::runByPixelsMask on the
 *                                                                           level-0 position (the per-level masks of
 *                                                                           cv::ORB are part of the E9 substitution)
 *   && nearEdges(kp): any contour pixel >= 10 in the box  row in [trunc(max(x-10,0)), min(x+10, cols)),
 *                     col in [trunc(max(y-10,0)), min(y+10, rows))  -- sic: the key point's X selects the image ROW and
 *                     is clamped with cols, its Y selects the COLUMN and is clamped with rows (Frame.cc:719-729); loop
 *                     bounds are float compares of a size_t counter, as in the reference.  On a non-square contour image
 *                     the reference reads out of bounds; here pixels outside the image count as 0 (free).
 * Survivors are appended in input order (push_back, Frame.cc:680); descriptors (computed before the filter in this
 * build, after it in the reference) move with their key points.  Outputs must not alias the inputs.
 * genEdgesPC (Frame.cc:686-715; lists nothing in the reference ever reads) is optional: edge_sign = pixels in [10,150),
 * edge_free = pixels >= 150, as (x = col, y = row) float pairs in raster order, at most edge_cap each (counts are
 * the true totals; entries beyond edge_cap are dropped). */
typedef struct fb_bird_guidance_args {
  int32_t batch, kp_stride;
  int32_t cols, rows, pitch;            /* mBirdviewContourICP / mBirdviewMask geometry; images rows*pitch bytes apart */
  const uint8_t *contour;               /* [batch][rows][pitch] u8                                               */
  const uint8_t *mask;                  /* optional, same geometry                                               */
  const int32_t *n_in;                  /* [batch]                                                               */
  const fb_keypoint *kps_in;            /* [batch][kp_stride]  preKeysBird (level-0 pixel coordinates)           */
  const uint8_t *desc_in;               /* optional [batch][kp_stride][32]                                       */
  int32_t *n_out;                       /* [batch]             Nbird                                             */
  fb_keypoint *kps_out;                 /* [batch][kp_stride]  mvKeysBird                                        */
  uint8_t *desc_out;                    /* [batch][kp_stride][32] (required iff desc_in)                         */
  uint8_t *keep;                        /* optional [batch][kp_stride]: 1 = survived                             */
  int32_t edge_cap;                     /* 0 = skip genEdgesPC                                                   */
  int32_t *n_edge_sign, *n_edge_free;   /* [batch]                                                               */
  float *edge_sign, *edge_free;         /* [batch][edge_cap][2]                                                  */
} fb_bird_guidance_args;
int fb_bird_guidance(const fb_bird_guidance_args *a);                    /* host pointers  */
int fb_bird_guidance_dev(const fb_bird_guidance_args *a, void *stream);  /* device pointers */

/* cv::cornerSubPix(mBirdviewImg, vKeysBird, Size(5,5), Size(-1,-1), {EPS+MAX_ITER, 40, 0.001}) (src/Frame.cc:345-352,
 * between GuidenceKeyBirdPts and the bird compute step): OpenCV 3's imgproc/src/cornersubpix.cpp with no zero zone, on a
 * u8 image, restated.  With w = half_win_x, h = half_win_y, per key point, start cT = (x, y), cI = cT, iter = 0:
 *   do {
 *     patch = getRectSubPix(image, (2w+3) x (2h+3), cI) as float (imgproc/src/samplers.cpp, 8u -> 32f): top-left corner
 *             t = cI - (size-1)*0.5f, ip = floor(t), (a, b) = t - ip (float); pixel (r, c) of the patch, with the source
 *             columns x0 = ip.x + c, x0 + 1 and rows y0 = ip.y + r, y0 + 1 each clamped into the image (replicate):
 *               0 <= x0 < cols-1 :  ((p00*a11 + p01*a12) + p10*a21) + p11*a22,  a11 = (1-a)(1-b), a12 = a(1-b),
 *                                                                               a21 = (1-a)b,     a22 = ab
 *               otherwise        :  p00*(1-b) + p10*b         (the border path's two-coefficient columns)
 *             float multiplies and adds in that order, none fused.
 *     over the (2w+1) x (2h+1) window, (i, j) row / column, px = j - w, py = i - h, in double:
 *       tgx = patch[i+1][j+2] - patch[i+1][j], tgy = patch[i+2][j+1] - patch[i][j+1]  (float differences)
 *       m = weight[i][j] = float(exp(-y*y)) * float(exp(-x*x)) as a float product, x = (j-w)/w, y = (i-h)/h in float
 *       gxx = tgx*tgx*m, gxy = tgx*tgy*m, gyy = tgy*tgy*m
 *       a += gxx, b += gxy, c += gyy, bb1 += gxx*px + gxy*py, bb2 += gxy*px + gyy*py
 *     det = a*c - b*b;  if (|det| <= DBL_EPSILON^2) break;                                     -- FB_SUBPIX_EXIT_DET
 *     scale = 1/det;  cI2 = float(cI.x + c*scale*bb1 - b*scale*bb2, cI.y - b*scale*bb1 + a*scale*bb2)
 *     err = (cI2.x-cI.x)^2 + (cI2.y-cI.y)^2 in float;  cI = cI2
 *     if (cI.x < 0 || cI.x >= cols || cI.y < 0 || cI.y >= rows) break;                         -- FB_SUBPIX_EXIT_OUT
 *   } while (++iter < max_iter                                                            -- else FB_SUBPIX_EXIT_ITER
 *            && err > eps*eps);                                                           -- else FB_SUBPIX_EXIT_EPS
 *   if (|cI.x - cT.x| > w || |cI.y - cT.y| > h) cI = cT;                                   -- | FB_SUBPIX_REVERTED
 * x / y of kps[b][i], i < n[b], are replaced by cI; no other byte of kps is written.  iters = `iter` on leaving the loop
 * (a round left by a break is not counted).  A point that left the image keeps its outside position unless the last rule
 * reverts it; the position is then at most w / h beyond the border.  The window sums are taken over the 64 lanes of a
 * wave, so they differ from a serial sum in the last bits; starts are expected to be finite. */
enum { FB_SUBPIX_EXIT_EPS = 0, FB_SUBPIX_EXIT_ITER = 1, FB_SUBPIX_EXIT_DET = 2, FB_SUBPIX_EXIT_OUT = 3, FB_SUBPIX_REVERTED = 4 };
typedef struct fb_corner_subpix_args {
  int32_t batch, kp_stride;
  int32_t cols, rows, pitch;            /* u8 image geometry; image b starts b * image_stride bytes after the base */
  size_t image_stride;
  const uint8_t *image;
  const int32_t *n;                     /* [batch]                                                               */
  fb_keypoint *kps;                     /* [batch][kp_stride]  x / y refined in place                            */
  int32_t half_win_x, half_win_y;       /* 1..8 (5, 5 in the reference)                                          */
  int32_t max_iter;                     /* 1..100 (40)                                                           */
  double eps;                           /* >= 0 (0.001); squared inside                                          */
  int32_t *iters;                       /* optional [batch][kp_stride]                                           */
  uint8_t *exit_code;                   /* optional [batch][kp_stride]  FB_SUBPIX_EXIT_* | FB_SUBPIX_REVERTED    */
} fb_corner_subpix_args;
int fb_corner_subpix(const fb_corner_subpix_args *a);                    /* host pointers  */
int fb_corner_subpix_dev(const fb_corner_subpix_args *a, void *stream);  /* device pointers */

/* ======================================================================== */
/* ORBmatcher (include/ORBmatcher.h:41-88, src/ORBmatcher.cc)                */
/* ======================================================================== */
typedef struct fb_matcher_params { /* ORBmatcher.h:41 */
  float nnratio;
  int32_t check_orientation;
} fb_matcher_params;

/* DescriptorDistance (ORBmatcher.cc:1951-1967): out[i] = popcount(a[i]^b[i]) over 32 bytes */
int fb_descriptor_distance_dev(const uint8_t *d_a, const uint8_t *d_b, int n, int32_t *d_out,
                               void *stream);
int fb_descriptor_distance(const uint8_t *a, const uint8_t *b, int n, int32_t *out);

/* Camera + frame constants used by the projection matchers (Frame.h statics) */
typedef struct fb_camera {
  float fx, fy, cx, cy;
  float min_x, min_y, max_x, max_y; /* mnMinX.. image bounds, Frame.cc:741-795 */
} fb_camera;

/* --- M3: SearchByProjection(Frame& cur, const Frame& last, th, bMono=true)
 *     (ORBmatcher.cc:1329-1471).  One problem per batch entry.  All arrays are
 *     [batch][stride] with the per-problem counts in n_cur / n_last.            */
typedef struct fb_proj_frame_args {
  int32_t batch;
  int32_t cur_stride;  /* entries per problem in the cur_* arrays            */
  int32_t last_stride; /* entries per problem in the last_* arrays           */
  /* current frame = search targets */
  const int32_t *n_cur;          /* [batch]                                   */
  const fb_keypoint *cur_kps;    /* mvKeysUn: x,y,octave,angle used            */
  const uint8_t *cur_desc;       /* mDescriptors rows                          */
  const int32_t *cur_cell_start; /* [batch][cols*rows+1]                       */
  const int32_t *cur_cell_items; /* [batch][cur_stride]                        */
  const uint8_t *cur_blocked;    /* mvpMapPoints[i] && Observations()>0 on entry; may be NULL */
  const float *cur_Tcw;          /* [batch][12] row-major 3x4 of mTcw          */
  /* last frame = queries */
  const int32_t *n_last;         /* [batch]                                   */
  const uint8_t *last_valid;     /* mvpMapPoints[i] && !mvbOutlier[i]          */
  const uint8_t *last_obs_pos;   /* pMP->Observations()>0                      */
  const float *last_xw;          /* [..][3] pMP->GetWorldPos()                 */
  const uint8_t *last_desc;      /* pMP->GetDescriptor()                       */
  const int32_t *last_octave;    /* LastFrame.mvKeys[i].octave                 */
  const float *last_angle;       /* LastFrame.mvKeysUn[i].angle                */
  /* constants */
  fb_camera cam;
  fb_grid_geom grid;
  float scale_factors[FB_MAX_LEVELS]; /* CurrentFrame.mvScaleFactors           */
  float th;
  fb_matcher_params matcher;
  /* outputs */
  int32_t *match_cur_to_last; /* [batch][cur_stride]: index into last, or -1   */
  int32_t *nmatches;          /* [batch] return value                          */
  /* Tracking.cc:1342-1349 in the same launch: a frame whose search returned fewer than retry_below matches (20 there) is
   * searched again from scratch with retry_th (2 * th there); match_cur_to_last / nmatches then hold the second result.
   * retry_below = 0: one search.                                              */
  int32_t retry_below;
  float retry_th;
  int32_t *retried;           /* [batch] or NULL: 1 = the second search ran     */
} fb_proj_frame_args;
int fb_match_projection_frame_dev(const fb_proj_frame_args *args, void *stream);
int fb_match_projection_frame(const fb_proj_frame_args *args); /* host pointers */

/* --- M9: BirdMapPointMatch(CurF, vRefMapPointsBird, windowSize, filterSize)
 *     (ORBmatcher.cc:1763-1902)                                               */
typedef struct fb_bird_mp_args {
  int32_t batch;
  int32_t cur_stride;
  int32_t ref_stride;
  const int32_t *n_cur;           /* mvKeysBird.size() == mDescriptorsBird.rows */
  const fb_keypoint *cur_kps;     /* mvKeysBird                                */
  const uint8_t *cur_desc;        /* mDescriptorsBird                          */
  const float *cur_cam_xyz;       /* [..][3] mvKeysBirdCamXYZ                  */
  const int32_t *cur_cell_start;  /* bird grid CSR                             */
  const int32_t *cur_cell_items;
  const float *cur_Tcw;           /* [batch][12]                               */
  const int32_t *n_ref;
  const uint8_t *ref_valid;       /* vRefMapPointsBird[i] != NULL              */
  const float *ref_xw;            /* [..][3]                                   */
  const uint8_t *ref_desc;
  float Tbc[12];                  /* Frame::Tbc rows 0..2 (Frame.cc:1018-1030) */
  int32_t bird_cols, bird_rows;   /* Frame::birdviewCols/Rows                  */
  double meter2pixel;             /* Frame.cc:41                               */
  double rear_axle_to_center;     /* Frame.cc:42                               */
  fb_grid_geom grid;              /* 32x32, min=0                              */
  int32_t window_size;
  float filter_size;
  fb_matcher_params matcher;
  int32_t *match_cur_to_ref;      /* [batch][cur_stride]: mvpMapPointsBird as ref index or -1 (in/out: pre-fill) */
  int32_t *ninliers;              /* [batch] return value                      */
} fb_bird_mp_args;
int fb_match_bird_mappoints_dev(const fb_bird_mp_args *args, void *stream);
int fb_match_bird_mappoints(const fb_bird_mp_args *args);

/* --- M2: SearchByProjection(Frame&, vector<MapPoint*>&, th) (ORBmatcher.cc:46-130) */
typedef struct fb_proj_points_args {
  int32_t batch;
  int32_t cur_stride;
  int32_t mp_stride;
  const int32_t *n_cur;
  const fb_keypoint *cur_kps;
  const uint8_t *cur_desc;
  const int32_t *cur_cell_start;
  const int32_t *cur_cell_items;
  const uint8_t *cur_blocked;    /* F.mvpMapPoints[idx] && Observations()>0 on entry */
  const int32_t *n_mp;
  const uint8_t *mp_track;       /* mbTrackInView && !isBad()                  */
  const uint8_t *mp_obs_pos;     /* pMP->Observations()>0                      */
  const float *mp_proj;          /* [..][2] mTrackProjX, mTrackProjY           */
  const int32_t *mp_level;       /* mnTrackScaleLevel                          */
  const float *mp_view_cos;      /* mTrackViewCos                              */
  const uint8_t *mp_desc;
  fb_grid_geom grid;
  float scale_factors[FB_MAX_LEVELS];
  float th;
  fb_matcher_params matcher;
  int32_t *match_cur_to_mp;      /* [batch][cur_stride] index into mp or -1     */
  int32_t *nmatches;
  /* optional device scratch of fb_match_projection_points_workspace(batch, mp_stride) bytes, 16-byte aligned, private to
   * this call until it has run: with it the grid walks and Hamming distances are computed once by many workgroups per
   * problem and only the serial "already taken" rule runs in one workgroup (same results; several times faster for the
   * few-thousand-point local maps of TrackLocalMap, above all at small batch).  NULL = the one-kernel version.        */
  void *workspace;
  size_t workspace_bytes;
} fb_proj_points_args;
size_t fb_match_projection_points_workspace(int batch, int mp_stride);
int fb_match_projection_points_dev(const fb_proj_points_args *args, void *stream);
int fb_match_projection_points(const fb_proj_points_args *args);

/* --- M8: BirdviewMatch(CurF, refKeys, refDesc, refMPBirds, matches, isProject=0, window)
 *     (ORBmatcher.cc:1602-1760), live form isProject=0.
 *     NOT BUILT: the isProject != 0 branch (ORBmatcher.cc:1617-1655: search centre = the reference MapPointBird projected
 *     with Tbc * Tcw, |z| <= 0.2 m gate, no level filter).  No call site of the reference uses it (Tracking.cc:384,407,
 *     450,959,2728 all pass 0); a caller that needs projected bird search has fb_match_bird_mappoints (M9), which is that
 *     projection + window search (BirdMapPointMatch, ORBmatcher.cc:1763-1902).                                        */
typedef struct fb_birdview_args {
  int32_t batch;
  int32_t cur_stride;
  int32_t ref_stride;
  const int32_t *n_cur;
  const fb_keypoint *cur_kps;
  const uint8_t *cur_desc;
  const int32_t *cur_cell_start;
  const int32_t *cur_cell_items;
  const int32_t *n_ref;
  const fb_keypoint *ref_kps;
  const uint8_t *ref_desc;
  fb_grid_geom grid;
  int32_t window_size;
  fb_matcher_params matcher;
  int32_t *match_ref_to_cur; /* [batch][ref_stride] vnMatches12 after culling (-1 = none) */
  int32_t *match_dist;       /* [batch][ref_stride] vMatchedDistance                      */
  int32_t *nmatches;         /* [batch] return value                                      */
  int32_t *n_dmatches;       /* [batch] number of DMatch emitted (vnMatches12[i] > 0)     */
} fb_birdview_args;
int fb_match_birdview_dev(const fb_birdview_args *args, void *stream);
int fb_match_birdview(const fb_birdview_args *args);

/* DBoW2::FeatureVector (Thirdparty/DBoW2/DBoW2/FeatureVector.h:23) = map<NodeId, vector<unsigned>> as CSR:
 * node ids ascending, node n owns items[node_start[n] .. node_start[n+1]) in addFeature order.          */
typedef struct fb_feature_vector {
  int32_t node_stride;        /* entries per problem in node_ids (node_start has node_stride+1)   */
  int32_t item_stride;        /* entries per problem in items                                      */
  const int32_t *n_nodes;     /* [batch]                                                            */
  const uint32_t *node_ids;   /* [batch][node_stride]                                               */
  const int32_t *node_start;  /* [batch][node_stride+1]                                             */
  const int32_t *items;       /* [batch][item_stride] feature indices                               */
} fb_feature_vector;

/* --- M5: SearchByBoW(KeyFrame* pKF, Frame &F, vector<MapPoint*>&) (ORBmatcher.cc:160-289) */
typedef struct fb_bow_args {
  int32_t batch;
  int32_t kf_stride, f_stride;
  const int32_t *n_kf;          /* pKF->N                                                            */
  const fb_keypoint *kf_kps;    /* pKF->mvKeysUn (angle)                                             */
  const uint8_t *kf_desc;
  const uint8_t *kf_has_mp;     /* vpMapPointsKF[i] && !isBad()                                      */
  fb_feature_vector kf_fv;      /* pKF->mFeatVec                                                     */
  const int32_t *n_f;           /* F.N                                                               */
  const fb_keypoint *f_kps;     /* F.mvKeys (angle)                                                  */
  const uint8_t *f_desc;
  fb_feature_vector f_fv;       /* F.mFeatVec                                                        */
  fb_matcher_params matcher;    /* ORBmatcher(0.7,true) at Tracking.cc:1207                          */
  int32_t *match_f_to_kf;       /* [batch][f_stride]: KF feature whose MapPoint lands in slot i, -1  */
  int32_t *nmatches;            /* [batch]                                                           */
} fb_bow_args;
int fb_match_bow_dev(const fb_bow_args *args, void *stream);
int fb_match_bow(const fb_bow_args *args);

/* --- M7: SearchForTriangulation(pKF1, pKF2, F12, pairs, bOnlyStereo=false) (ORBmatcher.cc:658-824) */
typedef struct fb_triangulation_args {
  int32_t batch;
  int32_t kf1_stride, kf2_stride;
  const int32_t *n1;
  const fb_keypoint *kps1;      /* pKF1->mvKeysUn                                                    */
  const uint8_t *desc1;
  const uint8_t *has_mp1;       /* pKF1->GetMapPoint(i) != NULL                                      */
  fb_feature_vector fv1;
  const int32_t *n2;
  const fb_keypoint *kps2;
  const uint8_t *desc2;
  const uint8_t *has_mp2;
  fb_feature_vector fv2;
  const float *F12;             /* [batch][9] row-major                                              */
  const float *Cw1;             /* [batch][3] pKF1->GetCameraCenter()                                */
  const float *R2w;             /* [batch][9] pKF2->GetRotation()                                    */
  const float *t2w;             /* [batch][3]                                                        */
  float fx, fy, cx, cy;         /* pKF2 intrinsics                                                   */
  float scale_factors[FB_MAX_LEVELS]; /* pKF2->mvScaleFactors                                        */
  float level_sigma2[FB_MAX_LEVELS];  /* pKF2->mvLevelSigma2                                         */
  fb_matcher_params matcher;    /* ORBmatcher(0.6,false) at LocalMapping.cc:239                      */
  int32_t *matches12;           /* [batch][kf1_stride] vMatches12                                    */
  int32_t *nmatches;            /* [batch]                                                           */
} fb_triangulation_args;
int fb_match_triangulation_dev(const fb_triangulation_args *args, void *stream);
int fb_match_triangulation(const fb_triangulation_args *args);

/* --- M4: SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound,
 *     th, ORBdist) (ORBmatcher.cc:1473-1600; relocalisation, Tracking.cc:1632,1643).              */
typedef struct fb_proj_kf_args {
  int32_t batch;
  int32_t cur_stride;
  int32_t kf_stride;
  const int32_t *n_cur;
  const fb_keypoint *cur_kps;    /* CurrentFrame.mvKeysUn                                            */
  const uint8_t *cur_desc;
  const int32_t *cur_cell_start;
  const int32_t *cur_cell_items;
  const uint8_t *cur_blocked;    /* CurrentFrame.mvpMapPoints[i2] != NULL on entry; may be NULL      */
  const float *cur_Tcw;          /* [batch][12]                                                      */
  const int32_t *n_kf;           /* vpMPs.size()                                                     */
  const uint8_t *kf_valid;       /* vpMPs[i] && !isBad() && !sAlreadyFound.count(vpMPs[i])           */
  const float *kf_xw;            /* [..][3] GetWorldPos()                                            */
  const uint8_t *kf_desc;        /* GetDescriptor()                                                  */
  const float *kf_max_dist;      /* mfMaxDistance (MapPoint.cc:379-383 applies the 1.2f)             */
  const float *kf_min_dist;      /* mfMinDistance (MapPoint.cc:373-377 applies the 0.8f)             */
  const float *kf_angle;         /* pKF->mvKeysUn[i].angle                                           */
  fb_camera cam;
  fb_grid_geom grid;
  float scale_factors[FB_MAX_LEVELS];
  float log_scale_factor;        /* CurrentFrame.mfLogScaleFactor                                    */
  int32_t n_levels;              /* CurrentFrame.mnScaleLevels                                       */
  float th;
  int32_t orb_dist;
  fb_matcher_params matcher;
  int32_t *match_cur_to_kf;      /* [batch][cur_stride]: index into the keyframe's points, or -1     */
  int32_t *nmatches;
} fb_proj_kf_args;
int fb_match_projection_keyframe_dev(const fb_proj_kf_args *args, void *stream);
int fb_match_projection_keyframe(const fb_proj_kf_args *args);

/* --- M6: SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12)
 *     (ORBmatcher.cc:523-656; loop closing, LoopClosing.cc:263).                                   */
typedef struct fb_bow_kf_args {
  int32_t batch;
  int32_t kf1_stride, kf2_stride;
  const int32_t *n1;            /* vpMapPoints1.size()                                               */
  const fb_keypoint *kps1;      /* pKF1->mvKeysUn (angle)                                            */
  const uint8_t *desc1;
  const uint8_t *has_mp1;       /* vpMapPoints1[i] && !isBad()                                       */
  fb_feature_vector fv1;
  const int32_t *n2;
  const fb_keypoint *kps2;
  const uint8_t *desc2;
  const uint8_t *has_mp2;       /* vpMapPoints2[i] && !isBad()                                       */
  fb_feature_vector fv2;
  fb_matcher_params matcher;    /* ORBmatcher(0.75,true) at LoopClosing.cc:240                       */
  int32_t *matches12;           /* [batch][kf1_stride]: KF2 feature whose MapPoint is vpMatches12[i], -1 */
  int32_t *nmatches;
} fb_bow_kf_args;
int fb_match_bow_kf_dev(const fb_bow_kf_args *args, void *stream);
int fb_match_bow_kf(const fb_bow_kf_args *args);

/* --- M10: the remaining ORBmatcher entry points (same windowed Hamming search) ------------------ */
/* key-frame side of a map-point -> key-frame search (KeyFrame.h members) */
typedef struct fb_kf_target {
  int32_t kf_stride;
  const int32_t *n_kf;            /* pKF->N                                                        */
  const fb_keypoint *kf_kps;      /* pKF->mvKeysUn                                                 */
  const uint8_t *kf_desc;         /* pKF->mDescriptors                                             */
  const int32_t *kf_cell_start;   /* pKF->mGrid as CSR (fb_grid_build_batch_dev)                   */
  const int32_t *kf_cell_items;
  fb_camera cam;                  /* fx, fy, cx, cy, mnMinX/Y, mnMaxX/Y                            */
  fb_grid_geom grid;
  float scale_factors[FB_MAX_LEVELS];    /* pKF->mvScaleFactors                                    */
  float inv_level_sigma2[FB_MAX_LEVELS]; /* pKF->mvInvLevelSigma2                                  */
  float log_scale_factor;         /* pKF->mfLogScaleFactor                                         */
  int32_t n_levels;               /* pKF->mnScaleLevels                                            */
} fb_kf_target;

/* candidate map points (MapPoint getters) */
typedef struct fb_mp_list {
  int32_t mp_stride;
  const int32_t *n_mp;
  const uint8_t *mp_valid;        /* the entry point's own skip rule, see each function             */
  const float *mp_xw;             /* [..][3] GetWorldPos()                                         */
  const float *mp_normal;         /* [..][3] GetNormal()                                           */
  const float *mp_max_dist;       /* mfMaxDistance                                                 */
  const float *mp_min_dist;       /* mfMinDistance                                                 */
  const uint8_t *mp_desc;         /* GetDescriptor()                                               */
} fb_mp_list;

/* Fuse(pKF, vpMapPoints, th) (ORBmatcher.cc:826-976; LocalMapping.cc:513,538) and
 * Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:978-1101; LoopClosing.cc:567).
 * The search half of Fuse: best_idx[i] = bestIdx if bestDist <= TH_LOW, else -1.  The map mutation that follows
 * (Replace / AddObservation / AddMapPoint, :950-971 and :1082-1096) stays with the caller, who walks best_idx in
 * order; the search result does not depend on those mutations.
 * mp_valid: Fuse = pMP && !isBad() && !IsInKeyFrame(pKF); Fuse-Sim3 = !isBad() && !spAlreadyFound.count(pMP).   */
typedef struct fb_fuse_args {
  int32_t batch;
  fb_kf_target kf;
  fb_mp_list mp;
  const float *pose;              /* [batch][12]: GetRotation|GetTranslation (Fuse) or rows 0..2 of Scw (Sim3) */
  const float *Ow;                /* [batch][3] GetCameraCenter() (Fuse); unused by the Sim3 variant  */
  float th;
  int32_t *best_idx;              /* [batch][mp_stride]                                             */
} fb_fuse_args;
int fb_fuse_search_dev(const fb_fuse_args *args, void *stream);
int fb_fuse_search(const fb_fuse_args *args);
int fb_fuse_sim3_search_dev(const fb_fuse_args *args, void *stream);
int fb_fuse_sim3_search(const fb_fuse_args *args);

/* SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (ORBmatcher.cc:291-404; LoopClosing.cc:377).
 * mp_valid = !isBad() && !spAlreadyFound.count(pMP).                                                 */
typedef struct fb_proj_sim3_args {
  int32_t batch;
  fb_kf_target kf;
  fb_mp_list mp;
  const float *Scw;               /* [batch][12]                                                    */
  const uint8_t *kf_matched;      /* vpMatched[idx] != NULL on entry                                */
  int32_t th;
  int32_t *match_kf_to_mp;        /* [batch][kf_stride]: point newly written to vpMatched[idx], or -1 */
  int32_t *nmatches;
} fb_proj_sim3_args;
int fb_match_projection_sim3_dev(const fb_proj_sim3_args *args, void *stream);
int fb_match_projection_sim3(const fb_proj_sim3_args *args);

/* SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (ORBmatcher.cc:1103-1327; LoopClosing.cc:341).
 * Per key-frame feature i: the MapPoint it holds (mp*.{xw,desc,max,min}[i]), mp*.mp_valid[i] =
 * vpMapPoints[i] && !vbAlreadyMatched[i] && !isBad().  kf1/kf2 strides equal mp1/mp2 strides.        */
typedef struct fb_sim3_args {
  int32_t batch;
  fb_kf_target kf1, kf2;
  fb_mp_list mp1, mp2;
  const float *T1w, *T2w;         /* [batch][12] GetRotation|GetTranslation of pKF1 / pKF2          */
  const float *s12;               /* [batch]                                                        */
  const float *R12;               /* [batch][9]                                                     */
  const float *t12;               /* [batch][3]                                                     */
  float th;
  int32_t *matches12;             /* [batch][kf1 stride]: idx2 with vnMatch1[i1]==idx2 && vnMatch2[idx2]==i1, or -1 */
  int32_t *nfound;
} fb_sim3_args;
int fb_match_sim3_dev(const fb_sim3_args *args, void *stream);
int fb_match_sim3(const fb_sim3_args *args);

/* SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (ORBmatcher.cc:406-521; Tracking.cc:1293) */
typedef struct fb_init_match_args {
  int32_t batch;
  int32_t f1_stride, f2_stride;
  const int32_t *n1;
  const fb_keypoint *kps1;        /* F1.mvKeysUn                                                    */
  const uint8_t *desc1;
  const int32_t *n2;
  const fb_keypoint *kps2;        /* F2.mvKeysUn                                                    */
  const uint8_t *desc2;
  const int32_t *f2_cell_start;   /* F2.mGrid                                                       */
  const int32_t *f2_cell_items;
  fb_grid_geom grid;
  int32_t window_size;
  fb_matcher_params matcher;      /* ORBmatcher(0.9,true) at Tracking.cc:1292                       */
  float *prev_matched;            /* [batch][f1_stride][2] vbPrevMatched, in/out                    */
  int32_t *matches12;             /* [batch][f1_stride] vnMatches12                                 */
  int32_t *nmatches;
} fb_init_match_args;
int fb_match_initialization_dev(const fb_init_match_args *args, void *stream);
int fb_match_initialization(const fb_init_match_args *args);

/* MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:242-307): for each map point, the observation descriptor with
 * the least median Hamming distance to the others.  CSR over map points: obs_start[n_mp+1], obs_desc[obs_start[n_mp]][32].
 * best_obs[i] = index (relative to obs_start[i]) of the chosen descriptor, -1 when the point has no observation. */
int fb_distinctive_descriptors_dev(const int32_t *d_obs_start, const uint8_t *d_obs_desc, int n_mp,
                                   int32_t *d_best_obs, void *stream);
int fb_distinctive_descriptors(const int32_t *obs_start, const uint8_t *obs_desc, int n_mp, int32_t *best_obs);

/* ======================================================================== */
/* LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:231-476)            */
/* ======================================================================== */
/* One key frame's new points: for each neighbour in GetBestCovisibilityKeyFrames(20) order the baseline / median-depth
 * gate, ComputeF12, SearchForTriangulation (M7, ORBmatcher(0.6,false)), and per match in ascending idx1 the parallax test,
 * the linear triangulation, the cheirality, chi2(2) and scale checks; then the point as MapPoint's constructor,
 * ComputeDistinctiveDescriptors and UpdateNormalAndDepth (pKF1 = reference key frame) leave it.
 * MONOCULAR ONLY: mvuRight = -1 for every key point (Frame.cc:252,323,799); the stereo / RGB-D branches
 * (LocalMapping.cc:270-274,325-346,368-375,396-436) are not built.  `if(i>0 && CheckNewKeyFrames()) return;` is not polled:
 * a caller that stops early passes fewer neighbours; the output of the first k neighbours is exactly the prefix of the
 * output of all of them.
 * Output rows: row k is the k-th `new MapPoint` of the reference (by neighbour, then ascending idx1); each KF1 feature
 * gets at most one point, so kf1_stride rows always suffice.  Two KF1 features may match the same neighbour slot
 * (vbMatched2 is never set): both become points and the slot holds the later one (kf2_new, has_mp2).
 * Pointers are DEVICE pointers for _dev, except nb_mp_start, which is a HOST array in both entry points (the caller
 * gathered the neighbours' points; the call validates it).  Errors: FB_ERR_ARG when matcher.check_orientation != 0
 * (the per-feature claim below needs M7 without the rotation histogram), when a neighbour has no map point (the
 * reference indexes an empty vector, KeyFrame.cc:994), when n_nb > FB_NEW_POINTS_MAX_NB, or when the workspace is
 * missing / too small (_dev).  n_nb = 0 writes n_new = 0 and kf1_new = -1.                                          */
#define FB_NEW_POINTS_MAX_NB 64
typedef struct fb_new_points_args {
  int32_t n_nb;                   /* neighbours, in covisibility order                                  */
  int32_t kf1_stride, kf2_stride;
  /* current key frame pKF1 */
  const int32_t *n1;              /* [1] pKF1->N                                                        */
  const fb_keypoint *kps1;        /* [kf1_stride] mvKeysUn                                              */
  const uint8_t *desc1;           /* [kf1_stride][32]                                                   */
  fb_feature_vector fv1;          /* batch 1                                                            */
  const float *Tcw1;              /* [12] GetRotation | GetTranslation, row-major 3x4                   */
  uint8_t *has_mp1;               /* in/out [kf1_stride]: GetMapPoint(i) != NULL                        */
  /* neighbours pKF2, strided like the KF2 side of fb_triangulation_args */
  const int32_t *n2;              /* [n_nb]                                                             */
  const fb_keypoint *kps2;        /* [n_nb][kf2_stride]                                                 */
  const uint8_t *desc2;           /* [n_nb][kf2_stride][32]                                             */
  fb_feature_vector fv2;          /* batch n_nb                                                         */
  const float *Tcw2;              /* [n_nb][12]                                                         */
  uint8_t *has_mp2;               /* in/out [n_nb][kf2_stride]                                          */
  const int32_t *nb_mp_start;     /* HOST [n_nb+1]: CSR over nb_mp_xw, every neighbour non-empty       */
  const float *nb_mp_xw;          /* [nb_mp_start[n_nb]][3]: non-NULL mvpMapPoints' GetWorldPos()      */
  const uint8_t *nb_before_kf1;   /* [n_nb]: (pKF2 < mpCurrentKeyFrame), the mObservations order       */
  /* camera (both key frames) and extractor tables */
  float fx, fy, cx, cy;
  float scale_factors[FB_MAX_LEVELS];
  float level_sigma2[FB_MAX_LEVELS];
  int32_t n_levels;               /* mnScaleLevels                                                      */
  float scale_factor;             /* mfScaleFactor                                                      */
  fb_matcher_params matcher;      /* ORBmatcher(0.6,false) at LocalMapping.cc:239                       */
  /* outputs, kf1_stride rows */
  int32_t *n_new;                 /* [1]                                                                */
  float *xw;                      /* [kf1_stride][3] GetWorldPos()      (fb_mp_list.mp_xw layout)       */
  float *normal;                  /* [kf1_stride][3] GetNormal()                                        */
  float *max_dist;                /* [kf1_stride] mfMaxDistance                                         */
  float *min_dist;                /* [kf1_stride] mfMinDistance                                         */
  uint8_t *desc;                  /* [kf1_stride][32] GetDescriptor()                                   */
  int32_t *idx1;                  /* [kf1_stride] observation in pKF1                                   */
  int32_t *nb;                    /* [kf1_stride] neighbour of the second observation                   */
  int32_t *idx2;                  /* [kf1_stride] its index in that neighbour                           */
  int32_t *kf1_new;               /* [kf1_stride] row of the point now in KF1 slot i, or -1             */
  int32_t *kf2_new;               /* [n_nb][kf2_stride] row of the point now in the slot (last writer), or -1 */
  int32_t *nb_matches;            /* [n_nb] SearchForTriangulation's return value for that neighbour    */
  int32_t *nb_new;                /* [n_nb] points created with that neighbour                          */
  int32_t *nb_skipped;            /* [n_nb] 1 = the baseline / median-depth gate skipped it             */
  /* device scratch of fb_create_new_map_points_workspace(n_nb, kf1_stride) bytes, 16-byte aligned, private to the
   * call until it has finished on `stream` (_dev only; the host drop-in allocates its own)                           */
  void *workspace;
  size_t workspace_bytes;
} fb_new_points_args;
size_t fb_create_new_map_points_workspace(int n_nb, int kf1_stride);
int fb_create_new_map_points_dev(const fb_new_points_args *args, void *stream);
int fb_create_new_map_points(const fb_new_points_args *args);

/* ======================================================================== */
/* Sim3Solver (src/Sim3Solver.cc; LoopClosing::ComputeSim3, LoopClosing.cc:225-420) */
/* ======================================================================== */
/* The RANSAC over Horn's closed form for every loop candidate of one key frame pKF1, in one call: the constructor
 * (:37-112), SetRansacParameters (:114-138) and ALL mRansacMaxIts iterations of iterate() (:140-231) per candidate, as a
 * table.  Iteration k of the reference depends on the earlier ones only through the running best count, so the table
 * holds every hypothesis (s, R, t, inlier count, inlier mask) plus the accept rule evaluated as a scan; a host that
 * replays iterate(n, ...) reads rows (mnIterations, mnIterations + n] of it (fishbird::Sim3Solver, fishbird_host.hpp).
 * The draws are an INPUT: rand_idx[c][k][j] is the value DUtils::Random::RandomInt(0, vAvailableIndices.size()-1)
 * returned for draw j of iteration k (:168), 0 <= rand_idx[c][k][j] <= N[c]-1-j; the swap-with-back removal (:175-176)
 * is replayed on the device.  Values outside that range are clamped into it (the range is the caller's contract).
 * MEMORY SAFETY, not in the reference (which would read out of bounds): a correspondence is also skipped, and so not counted
 * in N, when matches12[i1] >= the KF2 stride, when a GetIndexInKeyFrame value is >= its key frame's stride, or when the key
 * point it names has an octave outside [0, FB_MAX_LEVELS).  mRansacMaxIts is evaluated on the host with the reference's
 * expression (Sim3Solver.cc:125-135) for every N up to the KF1 stride and handed to the device as a step table.
 * MONOCULAR: the key frames' camera matrices are kf1.cam / kf2.cam (fx, fy, cx, cy).
 * Hypothesis rows are three separate tables so that &s[c][k], &R[c][k][0], &t[c][k][0] are the s12 / R12 / t12 of an
 * fb_sim3_args with batch 1.  Rows k >= max_its[c] are not written.  Pointers are DEVICE pointers for _dev.        */
#define FB_SIM3_MAX_HYP 300
typedef struct fb_sim3_corr {     /* one kept correspondence, compacted in ascending i1                       */
  float x3dc1[3];                 /* mvX3Dc1 = Rcw1*Xw1 + tcw1                                               */
  float x3dc2[3];                 /* mvX3Dc2                                                                 */
  float p1im1[2];                 /* mvP1im1 (FromCameraToImage, mK1)                                        */
  float p2im2[2];                 /* mvP2im2                                                                 */
  int32_t max_err1, max_err2;     /* mvnMaxError1/2 = (size_t)(9.210*mvLevelSigma2[octave]): TRUNCATED       */
} fb_sim3_corr;
typedef struct fb_sim3_solver_args {
  int32_t n_cand;                 /* candidates pKF2 of this call (nInitialCandidates), >= 1                 */
  fb_kf_target kf1;               /* pKF1, batch 1. Read: kf_stride, n_kf (= vpMatched12.size() = pKF1->N), kf_kps
                                     (mvKeysUn: octave), cam (mK1).  The other fields may be 0 / NULL.           */
  fb_kf_target kf2;               /* the candidates, batch n_cand ([n_cand][kf_stride] arrays). Same fields; mK2   */
  fb_mp_list mp1;                 /* per KF1 feature i1 (mp_stride == kf1.kf_stride): mp_valid = pMP1 && !isBad()
                                     with pMP1 = GetMapPointMatches()[i1]; mp_xw = GetWorldPos().  Rest unread.   */
  fb_mp_list mp2;                 /* per feature of each candidate ([n_cand][mp_stride], == kf2.kf_stride):
                                     mp_valid = !pMP2->isBad(); mp_xw                                           */
  const float *T1w;               /* [12] pKF1 GetRotation | GetTranslation, row-major 3x4                    */
  const float *T2w;               /* [n_cand][12]                                                            */
  const int32_t *kf1_index;       /* [kf1 stride] pMP1->GetIndexInKeyFrame(pKF1), or NULL = i1               */
  const int32_t *kf2_index;       /* [n_cand][kf2 stride] pMP2->GetIndexInKeyFrame(pKF2), or NULL = the slot */
  const int32_t *matches12;       /* [n_cand][kf1 stride]: KF2 feature whose point is vpMatched12[i1], or -1
                                     (what fb_match_bow_kf writes)                                           */
  float level_sigma2[FB_MAX_LEVELS]; /* mvLevelSigma2 (both key frames)                                      */
  int32_t fix_scale;              /* mbFixScale                                                              */
  double ransac_prob;             /* SetRansacParameters(probability, minInliers, maxIterations):            */
  int32_t min_inliers;            /*   (0.99, 20, 300) at LoopClosing.cc:278; min_inliers >= 3, any value    */
  int32_t max_iterations;         /*   1 .. FB_SIM3_MAX_HYP                                                  */
  const int32_t *accept_above;    /* [n_cand] or NULL = min_inliers: iterate returns when mnInliersi > this (:192).
                                     min(min_inliers, 15) restates the frame-id window of that line.          */
  const int32_t *rand_idx;        /* [n_cand][FB_SIM3_MAX_HYP][3] the RandomInt values, see above            */
  /* outputs per candidate */
  int32_t *N;                     /* [n_cand] N = mvpMapPoints1.size()                                       */
  int32_t *indices1;              /* [n_cand][kf1 stride] mvnIndices1 (rows < N)                             */
  fb_sim3_corr *corr;             /* [n_cand][kf1 stride] (rows < N), or NULL                                */
  int32_t *max_its;               /* [n_cand] mRansacMaxIts after SetRansacParameters                        */
  int32_t *n_hyp_done;            /* [n_cand] rows of the tables that were computed: max_its, 0 when N < min_inliers */
  int32_t *first_accept;          /* [n_cand] first k with accept, or -1: iterate returns at mnIterations = k+1 */
  int32_t *no_more;               /* [n_cand] 1 = N < min_inliers, or every iteration ran without a return (find() is empty) */
  /* outputs per (candidate, hypothesis k) */
  float *s;                       /* [n_cand][FB_SIM3_MAX_HYP]       ms12i                                    */
  float *R;                       /* [n_cand][FB_SIM3_MAX_HYP][9]    mR12i                                    */
  float *t;                       /* [n_cand][FB_SIM3_MAX_HYP][3]    mt12i                                    */
  int32_t *n_inliers;             /* [n_cand][FB_SIM3_MAX_HYP]       mnInliersi                               */
  uint8_t *accept;                /* [n_cand][FB_SIM3_MAX_HYP]       mnInliersi >= mnBestInliers && > accept_above */
  uint32_t *inlier_mask;          /* [n_cand][FB_SIM3_MAX_HYP][(kf1 stride+31)/32] mvbInliersi, bit i%32 of word i/32,
                                     compacted order (scatter through indices1); words < (N+31)/32 are written */
  /* device scratch of fb_sim3_solver_workspace(n_cand, kf1 stride) bytes, 16-byte aligned, private to the call until it
   * has finished on `stream` (_dev only; the host drop-in allocates its own)                                        */
  void *workspace;
  size_t workspace_bytes;
} fb_sim3_solver_args;
size_t fb_sim3_solver_workspace(int n_cand, int n1_stride);
int fb_sim3_solver_dev(const fb_sim3_solver_args *args, void *stream);  /* no host synchronisation */
int fb_sim3_solver(const fb_sim3_solver_args *args);                    /* host pointers */

/* Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) (src/Optimizer.cc:1560-1775; called at
 * LoopClosing.cc:341-360) for every candidate pKF2 of one pKF1 in one call, followed by mg2oScw = gScm * gSmw
 * (LoopClosing.cc:364-368).  kf1 / kf2 / mp1 / mp2 / T1w / T2w / kf2_index mean what they mean in fb_sim3_solver_args;
 * additionally kf_kps holds mvKeysUn's pt (the edges' measurements).  MONOCULAR: cam is fx, fy, cx, cy.
 * The seams of the reference, as implemented:
 *  - correspondence i1 is SKIPPED, and not counted in nCorrespondences, when matches12[i1] < 0, when pMP1 =
 *    GetMapPointMatches()[i1] is NULL or bad (mp1.mp_valid), when pMP2 is bad (mp2.mp_valid[matches12[i1]]), or when
 *    i2 = pMP2->GetIndexInKeyFrame(pKF2) < 0 (:1615-1650).  MEMORY SAFETY, not in the reference: matches12[i1] or i2 >= the KF2
 *    stride, or an octave (of mvKeysUn[i1] / pKF2->mvKeysUn[i2]) outside [0, FB_MAX_LEVELS), also skips; such a value is
 *    never used as an index.
 *  - P3Dc = R*Xw + t is a CV_32F product, ((r0*X + r1*Y) + r2*Z) + t without FMA (:1632,:1640), then widened to double;
 *    deltaHuber = sqrt(th2) is a float; invSigmaSquare is a float widened into the information matrix.
 *  - gScm = Sim3(toMatrix3d(R12), toVector3d(t12), s12): Quaterniond(R) in double from the floats, not normalised.
 *  - round 1 is optimize(5); a pair is bad if e12.chi2() > th2 || e21.chi2() > th2 (double chi2 against the float widened);
 *    bad pairs leave the graph and matches12[i1] = -1; nMoreIterations = nBad > 0 ? 10 : 5.
 *  - nCorrespondences - nBad < 10 returns 0: matches12 keeps the round-1 nulls and g2oS12 is NOT written back (:1745), so
 *    q / t / s hold the INPUT Sim3 and scw_* / Scw follow from it.  nCorrespondences == 0 returns 0 without a solve.
 *  - round 2 is initializeOptimization(); optimize(nMoreIterations) with a fresh lambda; the final check nulls matches12
 *    but removes nothing; n_inliers counts the rest.
 *  - the edges have no linearizeOplus (types_seven_dof_expmap.h:147,169), so the Jacobian is g2o's NUMERIC one: central
 *    differences with delta = 1e-9 through oplus on the Sim3 vertex (base_binary_edge.hpp:147-173).  oplusImpl zeroes
 *    update[6] IN the solver's x when fix_scale (types_seven_dof_expmap.h:60-70): column 6 of J is then exactly 0 and only
 *    the LM damping makes the 7x7 system regular.  LM is OptimizationAlgorithmLevenberg with LinearSolverDense.
 * Pointers are DEVICE pointers for _dev.                                                                            */
typedef struct fb_optimize_sim3_args {
  int32_t n_cand;                 /* candidates pKF2 of this call, >= 1                                       */
  fb_kf_target kf1;               /* pKF1, batch 1. Read: kf_stride, n_kf (= vpMatches1.size()), kf_kps, cam    */
  fb_kf_target kf2;               /* the candidates, batch n_cand. Read: kf_stride, kf_kps, cam                 */
  fb_mp_list mp1;                 /* per KF1 feature (mp_stride == kf1.kf_stride): mp_valid = pMP1 && !isBad(), mp_xw */
  fb_mp_list mp2;                 /* per feature of each candidate ([n_cand][kf2 stride]): mp_valid = !isBad(), mp_xw */
  const float *T1w;               /* [12] pKF1 GetRotation | GetTranslation, row-major 3x4                    */
  const float *T2w;               /* [n_cand][12]                                                            */
  const int32_t *kf2_index;       /* [n_cand][kf2 stride] pMP2->GetIndexInKeyFrame(pKF2), or NULL = the slot */
  float inv_level_sigma2[FB_MAX_LEVELS]; /* mvInvLevelSigma2 (both key frames)                                */
  int32_t *matches12;             /* IN/OUT [n_cand][kf1 stride]: KF2 feature whose point is vpMatches1[i1], or -1 (what
                                     fb_match_sim3 / fb_match_bow_kf write); set to -1 where the reference nulls vpMatches1 */
  const float *s12;               /* the input Sim3 of candidate c: s12[c * hyp_stride],                      */
  const float *R12;               /*   R12 + 9 * c * hyp_stride,                                              */
  const float *t12;               /*   t12 + 3 * c * hyp_stride                                               */
  int32_t hyp_stride;             /* 1 (or 0) = dense [n_cand] arrays as in fb_sim3_args; FB_SIM3_MAX_HYP = &s[0][k],
                                     &R[0][k][0], &t[0][k][0] of fb_sim3_solver's tables: row k of every candidate */
  float th2;                      /* 10 at LoopClosing.cc:360                                                */
  int32_t fix_scale;              /* mbFixScale                                                              */
  /* outputs per candidate */
  int32_t *n_inliers;             /* [n_cand] the return value                                               */
  int32_t *n_correspondences;     /* [n_cand] nCorrespondences                                               */
  int32_t *n_bad;                 /* [n_cand] nBad of the first round                                        */
  double *q, *t, *s;              /* [n_cand][4] (x, y, z, w), [n_cand][3], [n_cand]: g2oS12 on return        */
  double *scw_q, *scw_t, *scw_s;  /* mg2oScw = gScm * Sim3(R2w, t2w, 1): the q / t / s of fb_correct_loop_args */
  float *Scw;                     /* [n_cand][12] Converter::toCvMat(mg2oScw) rows 0..2, [s*R | t]: the Scw of
                                     fb_proj_sim3_args and the pose of fb_fuse_args (Sim3 variant)            */
  /* device scratch of fb_optimize_sim3_workspace(n_cand, kf1 stride) bytes, 16-byte aligned, private to the call until it
   * has finished on `stream` (_dev only; the host drop-in allocates its own)                                        */
  void *workspace;
  size_t workspace_bytes;
} fb_optimize_sim3_args;
size_t fb_optimize_sim3_workspace(int n_cand, int kf1_stride);
int fb_optimize_sim3_dev(const fb_optimize_sim3_args *args, void *stream);  /* enqueues only: no host synchronisation */
int fb_optimize_sim3(const fb_optimize_sim3_args *args);                    /* host pointers */

/* ======================================================================== */
/* DBoW2 vocabulary transform (Frame::ComputeBoW, src/Frame.cc:628-635)       */
/* ======================================================================== */
/* DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB> as flat arrays
 * (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:297-329: Node{weight, children, descriptor, word_id}, m_L).
 * The reference ships no vocabulary file; any tree (k, L) in this form works. */
typedef struct fb_vocabulary {
  int32_t n_nodes;
  int32_t L;                    /* m_L, depth of the leaves                                          */
  const int32_t *child_start;   /* [n_nodes+1] CSR over m_nodes[i].children                           */
  const int32_t *children;      /* NodeIds in the children vector's order                            */
  const uint8_t *descriptors;   /* [n_nodes][32]                                                      */
  const double *weights;        /* [n_nodes] Node::weight (used at the leaves)                        */
  const int32_t *word_ids;      /* [n_nodes] Node::word_id (used at the leaves)                       */
} fb_vocabulary;

/* transform(features, BowVector&, FeatureVector&, levelsup) for TF_IDF weighting + L1 scoring (ORBVocabulary),
 * TemplatedVocabulary.h:1126-1194, per-feature descent :1217-1259, BowVector::addWeight / normalize(L1)
 * (BowVector.cpp:30-84).  Outputs per image: the BowVector as (word id ascending, value) pairs and the FeatureVector
 * in the CSR form the matchers take (fb_feature_vector).  All output arrays have f_stride entries per image
 * (fv_node_start: f_stride + 1); entries at or beyond the returned counts (and below n_f) are scratch of the call. */
typedef struct fb_bow_transform_args {
  int32_t batch;
  int32_t f_stride;
  const int32_t *n_f;           /* features per image (<= 4096)                                       */
  const uint8_t *desc;          /* [batch][f_stride][32] mDescriptors                                 */
  int32_t levelsup;             /* 4 at Frame.cc:633                                                  */
  int32_t *n_words;             /* [batch] mBowVec.size()                                             */
  uint32_t *bow_ids;            /* [batch][f_stride]                                                  */
  double *bow_vals;             /* [batch][f_stride]                                                  */
  int32_t *fv_n_nodes;          /* [batch] mFeatVec.size()                                            */
  uint32_t *fv_node_ids;        /* [batch][f_stride]                                                  */
  int32_t *fv_node_start;       /* [batch][f_stride + 1]                                              */
  int32_t *fv_items;            /* [batch][f_stride]                                                  */
} fb_bow_transform_args;
int fb_bow_transform_dev(const fb_vocabulary *voc /* device arrays */, const fb_bow_transform_args *args, void *stream);
int fb_bow_transform(const fb_vocabulary *voc, const fb_bow_transform_args *args); /* host pointers */

/* ======================================================================== */
/* KeyFrameDatabase (src/KeyFrameDatabase.cc) and ORBVocabulary::score        */
/* ======================================================================== */
/* TemplatedVocabulary::score with L1 scoring (L1Scoring::score, Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) on
 * explicit pairs: score[i] = score(a_i, b_i) for [batch] BowVectors a and b (ids ascending, `stride` entries per vector).
 * The double sum runs over the shared words in ascending word order, exactly as the reference adds them.                */
int fb_bow_score_dev(int32_t batch, int32_t stride, const int32_t *na, const uint32_t *a_ids, const double *a_vals,
                     const int32_t *nb, const uint32_t *b_ids, const double *b_vals, double *score, void *stream);
int fb_bow_score(int32_t batch, int32_t stride, const int32_t *na, const uint32_t *a_ids, const double *a_vals,
                 const int32_t *nb, const uint32_t *b_ids, const double *b_vals, double *score); /* host pointers */

/* The reference's KeyFrameDatabase plus the six query members every KeyFrame carries for it (KeyFrame.h:157-162:
 * mnLoopQuery, mnLoopWords, mLoopScore, mnRelocQuery, mnRelocWords, mRelocScore).  A key frame is a slot in
 * [0, max_keyframes): the host's index for pKF, as the map tables of fb_track_args are indexed.  The BowVectors stay on
 * the device.  The handle is single-threaded, like fb_orb: the reference serialises its users with
 * KeyFrameDatabase::mMutex, here the caller serialises (or uses one stream).  Calls take effect in the order they are
 * made; occupancy errors are judged in that order.                                                                      */
typedef struct fb_kfdb fb_kfdb;
struct fb_frame;                /* the frame handle of the tracking chain below */
#define FB_KFDB_MAX_KEYFRAMES 4096
#define FB_KFDB_MAX_WORDS 4096
#define FB_KFDB_COVIS 10
typedef struct fb_kfdb_params {
  int32_t max_keyframes;        /* 1 .. FB_KFDB_MAX_KEYFRAMES                                          */
  int32_t word_stride;          /* words kept per BowVector, 1 .. FB_KFDB_MAX_WORDS                    */
} fb_kfdb_params;
int fb_kfdb_create(const fb_kfdb_params *p, fb_kfdb **out);
int fb_kfdb_destroy(fb_kfdb *db);
/* KeyFrameDatabase::clear (Tracking::Reset): every slot empty, the six members of every slot 0.                         */
int fb_kfdb_clear(fb_kfdb *db, void *stream);
/* KeyFrameDatabase::add(pKF).  The six members of the slot become 0 (KeyFrame.cc:35; the two scores, which the reference
 * leaves uninitialised, are defined as 0.0f).  The _dev variant keeps min(*d_n_words, word_stride) words.               */
int fb_kfdb_add_dev(fb_kfdb *db, int32_t slot, const int32_t *d_n_words, const uint32_t *d_bow_ids, const double *d_bow_vals,
                    void *stream);
int fb_kfdb_add(fb_kfdb *db, int32_t slot, int32_t n_words, const uint32_t *bow_ids, const double *bow_vals); /* host pointers */
/* add() of sequence 0 of a frame handle after fb_frame_compute_bow_dev (needs kp_stride <= word_stride).                */
int fb_kfdb_add_frame_dev(fb_kfdb *db, int32_t slot, struct fb_frame *kf, void *stream);
/* KeyFrameDatabase::erase(pKF) (KeyFrame::SetBadFlag): the slot's six members stay, as they do on the bad KeyFrame.     */
int fb_kfdb_erase(fb_kfdb *db, int32_t slot, void *stream);

enum { FB_KFDB_RELOC = 0, FB_KFDB_LOOP = 1 };
typedef struct fb_kfdb_query_args {
  int32_t mode;                 /* FB_KFDB_RELOC: DetectRelocalizationCandidates(F) (KeyFrameDatabase.cc:199-309);
                                   FB_KFDB_LOOP: DetectLoopCandidates(pKF, minScore) (:76-197)            */
  uint64_t query_id;            /* F->mnId / pKF->mnId                                                  */
  const int32_t *n_words;       /* [1]  the query's mBowVec                                             */
  const uint32_t *bow_ids;      /* [n_words] ascending                                                  */
  const double *bow_vals;       /* [n_words]                                                            */
  float min_score;              /* LOOP                                                                 */
  int32_t n_connected;          /* LOOP: entries of `connected`                                         */
  const int32_t *connected;     /* LOOP: slots of pKF->GetConnectedKeyFrames() (may be NULL when n_connected == 0) */
  const int32_t *covis;         /* [max_keyframes][FB_KFDB_COVIS] slots of GetBestCovisibilityKeyFrames(10) per key
                                   frame in the vector's order, -1 = no entry                           */
  int32_t *n_candidates;        /* [1]                                                                  */
  int32_t *candidates;          /* [max_keyframes] slots, in the order of the returned vector           */
  /* optional (NULL = not wanted): what the reference computes on the way */
  int32_t *n_sharing;           /* [1] lKFsSharingWords.size()                                          */
  int32_t *max_common_words;    /* [1] maxCommonWords (0 when the list is empty)                        */
  int32_t *n_scored;            /* [1] nscores                                                          */
  int32_t *common_words;        /* [max_keyframes] mn{Loop,Reloc}Words of every slot after the call     */
  float *scores;                /* [max_keyframes] m{Loop,Reloc}Score of every slot after the call      */
} fb_kfdb_query_args;
int fb_kfdb_query_dev(fb_kfdb *db, const fb_kfdb_query_args *args, void *stream);  /* no synchronisation */
int fb_kfdb_query(fb_kfdb *db, const fb_kfdb_query_args *args);                    /* host pointers */

/* LoopClosing::DetectLoop's reference score (LoopClosing.cc:127-141): scores[i] = (float)score(query, slots[i]) for a
 * list of slots, *min_score = the minimum over those with skip[i] == 0 (skip = pKF->isBad(); NULL = none skipped),
 * starting from 1.  A slot's BowVector outlives erase (the bad KeyFrame keeps its mBowVec) until the slot is added again.
 * scores may be NULL.                                                                                                   */
int fb_kfdb_min_score_dev(fb_kfdb *db, const int32_t *d_n_words, const uint32_t *d_bow_ids, const double *d_bow_vals,
                          int32_t n_list, const int32_t *d_slots, const uint8_t *d_skip, float *d_scores, float *d_min_score,
                          void *stream);
int fb_kfdb_min_score(fb_kfdb *db, int32_t n_words, const uint32_t *bow_ids, const double *bow_vals, int32_t n_list,
                      const int32_t *slots, const uint8_t *skip, float *scores, float *min_score); /* host pointers */

/* ======================================================================== */
/* Covisibility graph (src/KeyFrame.cc) and LocalMapping::KeyFrameCulling     */
/* ======================================================================== */
/* The caller's map as device arrays; read-only to the library, like fb_map_points.  Preconditions: a (mp, kf) pair occurs
 * at most once among the live edges (it is a std::map key); kf_order is distinct over the slots in use; the configuration
 * is monocular, so MapPoint::Observations() is the number of live edges of the point (mvuRight < 0, MapPoint.cc:119-122).
 * An edge whose obs_kf >= max_keyframes, whose obs_mp or obs_idx is out of range, or a kf_mp entry >= n_mp is skipped on
 * the device, never used as an index, and counted (fb_covis_error_count).                                               */
typedef struct fb_covis_map {
  int32_t max_keyframes;        /* slots, as fb_kfdb: the host's index for pKF; equals the handle's max_keyframes      */
  int32_t kp_stride;            /* 1 .. FB_COVIS_MAX_STRIDE                                                            */
  const int32_t *kf_n;          /* [max_keyframes] N (0 for an unused slot)                                            */
  const int32_t *kf_mp;         /* [max_keyframes][kp_stride] mvpMapPoints[i] as a map point index, -1 = NULL          */
  const uint8_t *kf_octave;     /* [max_keyframes][kp_stride] mvKeysUn[i].octave                                       */
  int32_t n_mp;
  const uint8_t *mp_bad;        /* [n_mp] isBad()                                                                      */
  int32_t n_obs;                /* all MapPoint::mObservations of the map as one edge list, any order:                 */
  const int32_t *obs_mp, *obs_kf, *obs_idx;  /* [n_obs]; obs_kf < 0: erased entry (append / tombstone friendly; the same
                                   shape as fb_local_ba_args.obs_*)                                                    */
  const uint64_t *kf_order;     /* [max_keyframes] the key std::map<KeyFrame*,..> orders by: (uintptr_t)pKF            */
} fb_covis_map;
#define FB_COVIS_MAX_STRIDE 32767 /* a weight is at most kp_stride and is kept in 15 bits                              */
#define FB_COVIS_TH 15            /* th of KeyFrame::UpdateConnections (KeyFrame.cc:621)                               */

/* mConnectedKeyFrameWeights and the membership of mvpOrderedConnectedKeyFrames of every key frame (slot).  The ordered
 * vector is always "descending by (weight, kf_order)" over its members (KeyFrame.cc:202-209, :648-655) and is derived on
 * read.  Until an order is given (fb_covis_set_order_dev, or any call that takes a fb_covis_map) slots order by index.
 * Every call below enqueues on `stream`, none synchronises, and they take effect in call order; the handle is
 * single-threaded like fb_kfdb.  The calls that take a fb_covis_map use scratch owned by the handle: it grows on demand
 * (a growing call waits for the device once), or is sized ahead with fb_covis_reserve.                                   */
typedef struct fb_covis fb_covis;
int fb_covis_create(int32_t max_keyframes /* 1 .. FB_KFDB_MAX_KEYFRAMES */, fb_covis **out);
int fb_covis_destroy(fb_covis *g);
int fb_covis_clear(fb_covis *g, void *stream);          /* every row empty, the error counter 0                        */
int fb_covis_reserve(fb_covis *g, int32_t n_mp, int32_t n_obs, int32_t n_q);
int fb_covis_set_order_dev(fb_covis *g, const uint64_t *d_kf_order /* [max_keyframes] */, void *stream);
/* entries skipped on the device since creation / clear (see fb_covis_map); waits for `stream`                           */
int fb_covis_error_count(fb_covis *g, int32_t *count, void *stream);

/* KeyFrame::UpdateConnections (KeyFrame.cc:564-663) for the n_q key frames d_slots[0..n_q), with the result of calling
 * them one after another in list order.  Row a becomes the counter (entries below FB_COVIS_TH included); the members of
 * its ordered list are the entries >= FB_COVIS_TH, or pKFmax alone (the smallest kf_order among the maxima, :627-643);
 * every member b gets AddConnection(a, w).  An empty counter changes nothing (:604-612).  d_n_counter[q] =
 * KFcounter.size(), d_front[q] = mvpOrderedConnectedKeyFrames.front() afterwards (-1: the vector is empty).  The spanning
 * tree (mpParent, mbFirstConnection) follows with fb_covis_first_connection_dev, and the UpdateBirdConnections that ends
 * the function (:701, :608-609) with fb_covis_update_bird_connections_dev on the same batch.                            */
int fb_covis_update_connections_dev(fb_covis *g, const fb_covis_map *map, int32_t n_q, const int32_t *d_slots,
                                    int32_t *d_n_counter, int32_t *d_front, void *stream);
int fb_covis_update_connections(fb_covis *g, const fb_covis_map *map, int32_t n_q, const int32_t *slots, int32_t *n_counter,
                                int32_t *front); /* host pointers, the map's arrays included */
/* slot->AddConnection(other, weight) (KeyFrame.cc:179-192; weight 1 .. FB_COVIS_MAX_STRIDE) and
 * slot->EraseConnection(other) (:885-899): the ordered list is rebuilt from every entry only if the row changed.        */
int fb_covis_add_connection_dev(fb_covis *g, int32_t slot, int32_t other, int32_t weight, void *stream);
int fb_covis_erase_connection_dev(fb_covis *g, int32_t slot, int32_t other, void *stream);
/* the graph part of KeyFrame::SetBadFlag (:797-798, :807-808): EraseConnection(slot) on every key frame of its row, then
 * the row and its ordered list are cleared                                                                              */
int fb_covis_erase_keyframe_dev(fb_covis *g, int32_t slot, void *stream);

/* Getters.  d_slots / d_weights hold max_keyframes entries; entries past *d_n are left as they are.                     */
/* GetVectorCovisibleKeyFrames + mvOrderedWeights (d_weights may be NULL); GetBestCovisibilityKeyFrames(N) is the prefix */
int fb_covis_ordered_dev(fb_covis *g, int32_t slot, int32_t *d_n, int32_t *d_slots, int32_t *d_weights, void *stream);
int fb_covis_ordered(fb_covis *g, int32_t slot, int32_t *n, int32_t *slots, int32_t *weights);
/* GetCovisiblesByWeight(w) (:246-261): the prefix with weight >= w, and EMPTY when every weight is >= w (upper_bound
 * returns end()), as in the reference                                                                                   */
int fb_covis_by_weight_dev(fb_covis *g, int32_t slot, int32_t w, int32_t *d_n, int32_t *d_slots, void *stream);
int fb_covis_by_weight(fb_covis *g, int32_t slot, int32_t w, int32_t *n, int32_t *slots);
/* GetConnectedKeyFrames (a std::set: ascending kf_order); the `connected` argument of fb_kfdb_query_dev                 */
int fb_covis_connected_dev(fb_covis *g, int32_t slot, int32_t *d_n, int32_t *d_slots, void *stream);
int fb_covis_connected(fb_covis *g, int32_t slot, int32_t *n, int32_t *slots);
/* slot->GetWeight(other) (:263-270)                                                                                     */
int fb_covis_weight_dev(fb_covis *g, int32_t slot, int32_t other, int32_t *d_weight, void *stream);
int fb_covis_weight(fb_covis *g, int32_t slot, int32_t other, int32_t *weight);
/* rows [max_keyframes][FB_KFDB_COVIS] of GetBestCovisibilityKeyFrames(10), -1 padded, as fb_kfdb_query_args.covis reads
 * them: the rows of the n slots listed (d_slots == NULL: every row, n ignored); other rows are left as they are         */
int fb_covis_kfdb_rows_dev(fb_covis *g, int32_t n, const int32_t *d_slots, int32_t *d_covis, void *stream);
int fb_covis_kfdb_rows(fb_covis *g, int32_t n, const int32_t *slots, int32_t *covis);

/* LocalMapping::KeyFrameCulling (LocalMapping.cc:656-729) over GetVectorCovisibleKeyFrames() of cur_slot, in that order,
 * with the effects of each SetBadFlag() on the key frames after it: the culled key frame's observation edges are gone,
 * every point it observed loses one observation, and a point that drops to <= 2 is bad (MapPoint.cc:129-136).  These
 * effects live in scratch of the call: the map and the graph are not modified.  id0_slot (mnId == 0, :667; -1 = none)
 * is skipped with zeros; d_not_erase[slot] (mbNotErase, KeyFrame.cc:790-794; NULL = none) keeps a culled key frame
 * without effect.  Outputs in list order: d_slots, d_n_redundant, d_n_mps [max_keyframes] int32, d_culled
 * [max_keyframes] uint8 (nRedundantObservations > 0.9 * nMPs), and d_mp_bad_after [n_mp].                              */
int fb_covis_keyframe_culling_dev(fb_covis *g, const fb_covis_map *map, int32_t cur_slot, int32_t id0_slot,
                                  const uint8_t *d_not_erase, int32_t *d_n, int32_t *d_slots, int32_t *d_n_redundant,
                                  int32_t *d_n_mps, uint8_t *d_culled, uint8_t *d_mp_bad_after, void *stream);
int fb_covis_keyframe_culling(fb_covis *g, const fb_covis_map *map, int32_t cur_slot, int32_t id0_slot, const uint8_t *not_erase,
                              int32_t *n, int32_t *slots, int32_t *n_redundant, int32_t *n_mps, uint8_t *culled,
                              uint8_t *mp_bad_after); /* host pointers, the map's arrays included */

/* ---- the local-BA window (head and tail of Optimizer::LocalBundleAdjustment[WithOdom], Optimizer.cc:838-889,
 * :2139-2227, the edge loops :2312-2417, the write-back :2574-2669) ----------------------------------------------------
 * The caller's per-key-frame and per-point tables next to fb_covis_map.  Read-only for fb_covis_local_window_dev;
 * fb_covis_window_scatter_dev writes kf_Tcw, mp_xw and mpb_xw.  The bird side mirrors fb_covis_map for MapPointBird and is
 * skipped when bobs_kf is NULL; its tombstone and out-of-range rules are those of the front edge list.                  */
typedef struct fb_covis_kf_tables {
  float *kf_Tcw;                  /* [max_keyframes][12]                                                               */
  const uint8_t *kf_bad;          /* [max_keyframes] isBad()                                                           */
  const uint8_t *kf_init;         /* [max_keyframes] isInit (Optimizer.cc:2260)                                        */
  const fb_keypoint *kf_keys_un;  /* [max_keyframes][kp_stride] mvKeysUn (x, y, octave are read)                       */
  int32_t n_levels;               /* 1 .. FB_MAX_LEVELS                                                                */
  const float *inv_level_sigma2;  /* [n_levels] mvInvLevelSigma2; an octave outside [0, n_levels) is clamped + counted */
  float *mp_xw;                   /* [map.n_mp][3] GetWorldPos()                                                       */
  int32_t bird_stride;            /* 1 .. FB_COVIS_MAX_STRIDE                                                          */
  const int32_t *kf_nb;           /* [max_keyframes] mvKeysBird.size()                                                 */
  const int32_t *kf_mpb;          /* [max_keyframes][bird_stride] mvpMapPointsBird[i] as an index, -1 = NULL           */
  const uint8_t *kf_bird_octave;  /* [max_keyframes][bird_stride] mvKeysBird[i].octave (:2404)                         */
  const float *kf_bird_xc;        /* [max_keyframes][bird_stride][3] mvKeysBirdCamXYZ                                  */
  int32_t n_mpb;
  const uint8_t *mpb_bad;         /* [n_mpb]                                                                           */
  float *mpb_xw;                  /* [n_mpb][3]                                                                        */
  int32_t n_bobs;
  const int32_t *bobs_mpb, *bobs_kf, *bobs_idx;  /* [n_bobs]; bobs_kf < 0: erased entry                                */
} fb_covis_kf_tables;

typedef struct fb_covis_window_header {
  int32_t n_local, n_fixed, n_mp, n_obs, n_mpb, n_bobs;
  int32_t overflow;               /* != 0: a list did not fit its capacity; what fitted is written, nothing past it    */
} fb_covis_window_header;

/* The window as caller-provided arrays with their capacities: everything fb_local_ba_args needs except the odometry
 * edges.  Key frames: the local ones in lLocalKeyFrames order (cur, then GetVectorCovisibleKeyFrames() without the bad
 * ones), then the fixed ones in lFixedCameras order.  Points in lLocalMapPoints order.  Edges grouped by point in that
 * order, within a point in ascending kf_order, edges of bad key frames left out (:2332, :2392).  The bird arrays may be
 * NULL (cap_mpb = cap_bobs = 0) when the call is made without the bird side.                                            */
typedef struct fb_covis_window {
  int32_t cap_kf, cap_mp, cap_obs, cap_mpb, cap_bobs;
  int32_t *kf_slot;               /* [cap_kf]                                                                          */
  uint8_t *kf_fixed;              /* [cap_kf] isInit of a local key frame, 1 for a fixed one                           */
  float *kf_Tcw;                  /* [cap_kf][12] gathered                                                             */
  int32_t *mp_index;              /* [cap_mp] map point indices                                                        */
  float *mp_xw;                   /* [cap_mp][3] gathered                                                              */
  int32_t *obs_kf, *obs_mp;       /* [cap_obs] indices into kf_slot / mp_index                                         */
  int32_t *obs_src;               /* [cap_obs] the edge's index in the map's edge list                                 */
  float *obs_uv;                  /* [cap_obs][2] mvKeysUn[idx].pt                                                     */
  float *obs_inv_sigma2;          /* [cap_obs]                                                                         */
  int32_t *mpb_index;             /* [cap_mpb]                                                                         */
  float *mpb_xw;                  /* [cap_mpb][3]                                                                      */
  int32_t *bobs_kf, *bobs_mpb, *bobs_src; /* [cap_bobs]                                                                */
  float *bobs_xc;                 /* [cap_bobs][3] mvKeysBirdCamXYZ[idx]                                               */
  float *bobs_inv_sigma2;         /* [cap_bobs]                                                                        */
  fb_covis_window_header *header; /* [1]                                                                               */
} fb_covis_window;

/* Scratch for the window calls, ahead of time (they grow it on demand like the other map calls): the map's sizes as
 * for fb_covis_reserve, plus the bird side's (0, 0 without it).                                                         */
int fb_covis_reserve_window(fb_covis *g, int32_t n_mp, int32_t n_obs, int32_t n_mpb, int32_t n_bobs);

/* Collects the window of cur_slot from the graph's current rows and the map (device pointers throughout); enqueues only.
 * Local points: the local key frames in list order, features ascending, the first occurrence of each non-NULL, non-bad
 * point (:2156-2170).  Fixed key frames: the local points in order, each point's observers in ascending kf_order, the
 * first occurrence of a key frame that is not in the neighbour list; a bad neighbour is in neither list (it is marked at
 * :2149 before the isBad test), a bad observer is marked and not listed (:2181-2186); with_bird != 0 continues the fixed
 * list with the bird walk (:2213-2226).  Precondition: cur_slot is not the key frame with mnId == 0 (for it the
 * reference's initial mnBA*ForKF == 0 marks make the window degenerate, and LocalMapping::Run never optimises it).
 * Out-of-range entries are skipped and counted as in the other map calls.                                              */
int fb_covis_local_window_dev(fb_covis *g, const fb_covis_map *map, const fb_covis_kf_tables *tables, int32_t cur_slot,
                              int32_t with_bird, const fb_covis_window *out, void *stream);
/* The one synchronisation: the header of the handle's last fb_covis_local_window_dev, and kf_slot / kf_fixed (host
 * arrays of that call's cap_kf entries, either may be NULL; entries past n_local + n_fixed are -1 / 0), which
 * fb_local_ba_dev and the host's odometry chain need.  FB_ERR_CAPACITY when the window overflowed a capacity.
 * The header lives in the handle's scratch until a later call writes there: any map-taking call that builds its index
 * (fb_covis_update_connections*, fb_covis_keyframe_culling*, fb_covis_process_new_keyframe*, fb_covis_map_point_culling*,
 * and local_map / correct_loop / refresh_points unless reuse_index = 1 reuses the window's index), a call that grows the
 * scratch, or the next window.  After one of them, and before the first window, this call is FB_ERR_ARG.                 */
int fb_covis_local_window_header(fb_covis *g, fb_covis_window_header *header, int32_t *kf_slot, uint8_t *kf_fixed, void *stream);
/* host pointers throughout (out->header included); FB_ERR_CAPACITY as above                                             */
int fb_covis_local_window(fb_covis *g, const fb_covis_map *map, const fb_covis_kf_tables *tables, int32_t cur_slot,
                          int32_t with_bird, const fb_covis_window *out);

/* After the optimisation (:2574-2669), on the window's device arrays: kf_Tcw of the LOCAL key frames and mp_xw / mpb_xw
 * go back into the tables by slot / index, and the edges flagged in d_obs_outlier / d_bobs_outlier (fb_local_ba_args;
 * NULL = none) are compacted in edge order into d_erase / d_berase as rows (key frame slot, point index, feature index,
 * edge index in the map's list), [cap_obs][4] / [cap_bobs][4], their counts in d_n_erase[0] / d_n_erase[1].
 * EraseMapPointMatch, EraseObservation and UpdateNormalAndDepth stay with the host on those lists.                      */
int fb_covis_window_scatter_dev(fb_covis *g, const fb_covis_map *map, const fb_covis_kf_tables *tables, const fb_covis_window *win,
                                const uint8_t *d_obs_outlier, const uint8_t *d_bobs_outlier, int32_t *d_n_erase,
                                int32_t *d_erase, int32_t *d_berase, void *stream);

/* ---- the spanning tree (mpParent, mspChildrens, mbFirstConnection; KeyFrame.cc:665-690, :704-741, :810-868) ------------
 * State per slot: parent (int32, -1 = mpParent == NULL), linked (uint8: the slot is in mspChildrens of parent[slot]) and
 * first (uint8 = mbFirstConnection; 1 after create / clear).  GetChilds() of a non-bad key frame a is
 * {c : parent[c] == a && linked[c]} in ascending kf_order (a std::set<KeyFrame*>).  linked is there because SetBadFlag
 * leaves mpParent of the removed key frame set but erases it from its parent's set (:868).  ChangeParent adds to the new
 * set without erasing from the old one (:724-729); the old parent is then the key frame that is going bad, and the
 * children set of a key frame that has gone bad is not kept: nothing reachable reads it.  fb_covis_clear resets the tree.
 * Every call enqueues on `stream`; the host variants wait for the default stream.                                       */
/* the three arrays, whole ([max_keyframes] each; a NULL array is left out).  A parent outside [-1, max_keyframes) is
 * stored as -1 and counted.                                                                                             */
int fb_covis_tree_set_dev(fb_covis *g, const int32_t *d_parent, const uint8_t *d_linked, const uint8_t *d_first, void *stream);
int fb_covis_tree_get_dev(fb_covis *g, int32_t *d_parent, uint8_t *d_linked, uint8_t *d_first, void *stream);
int fb_covis_tree_get(fb_covis *g, int32_t *parent, uint8_t *linked, uint8_t *first); /* host pointers; synchronises     */
/* slot->ChangeParent(parent) (:724-729).  (The parents UpdateBirdConnections sets, :468-556, are set on the device by
 * fb_covis_update_bird_connections_dev.)                                                                                */
int fb_covis_change_parent_dev(fb_covis *g, int32_t slot, int32_t parent, void *stream);
/* parent->EraseChild(slot) (:718-722): linked is cleared only if parent[slot] == parent                                 */
int fb_covis_erase_child_dev(fb_covis *g, int32_t parent, int32_t slot, void *stream);
/* GetChilds() in set order (d_slots holds max_keyframes entries; entries past *d_n are left as they are) / GetParent()  */
int fb_covis_children_dev(fb_covis *g, int32_t slot, int32_t *d_n, int32_t *d_slots, void *stream);
int fb_covis_children(fb_covis *g, int32_t slot, int32_t *n, int32_t *slots);
int fb_covis_parent_dev(fb_covis *g, int32_t slot, int32_t *d_parent, void *stream);
/* The mbFirstConnection block of UpdateConnections (:665-690), on the outputs of fb_covis_update_connections_dev for the
 * same batch, in list order.  Query q acts only when first[slot] != 0, slot != id0_slot (mnId == 0; -1 = none) and
 * d_n_counter[q] != 0 (an empty counter returned at :604-612, mbFirstConnection stays set; d_front is then the front of
 * the unchanged vector and says nothing).  Then parent = d_front[q], or, when now_state4 != 0 and
 * frame_id[front] > frame_id[slot], this fork's override (:673-684): the key frame of the map (d_kf_in_map[slot] != 0)
 * with the largest mnFrameId strictly between 0 and this key frame's (frame id 0 never wins: the comparison is > 0; the
 * smaller kf_order among equal ids); if nothing qualifies the front stays.  linked = 1, first = 0.  d_kf_frame_id
 * [max_keyframes] int32 and d_kf_in_map [max_keyframes] uint8 may be NULL when now_state4 == 0.                         */
int fb_covis_first_connection_dev(fb_covis *g, int32_t n_q, const int32_t *d_slots, const int32_t *d_n_counter,
                                  const int32_t *d_front, int32_t id0_slot, int32_t now_state4, const int32_t *d_kf_frame_id,
                                  const uint8_t *d_kf_in_map, void *stream);
/* The tree part of KeyFrame::SetBadFlag (:810-868).  Independent of fb_covis_erase_keyframe_dev (the key frame itself is
 * never a parent candidate): the two may be called in either order.  Candidates = {parent[slot]}.  Repeatedly, over the
 * linked children in ascending kf_order (bad ones, d_kf_bad[c] != 0, skipped) and each child's ordered list in list
 * order, the pair (child, member that is a candidate) with the largest GetWeight under strict > (the first pair in that
 * order wins a tie) is re-parented, the child joins the candidates and leaves the set; when no pair is left, the
 * remaining children, bad ones included, get ChangeParent(parent[slot]) (:862-866).  Then linked[slot] = 0; parent[slot]
 * is kept.  Precondition parent[slot] >= 0 (the reference dereferences it): otherwise nothing is done and the error
 * counter goes up.  mnId == 0 / mbNotErase stay the caller's decision, as for fb_covis_erase_keyframe_dev.             */
int fb_covis_tree_erase_keyframe_dev(fb_covis *g, int32_t slot, const uint8_t *d_kf_bad, void *stream);

/* ---- Tracking::UpdateLocalMap = UpdateLocalKeyFrames + UpdateLocalPoints (Tracking.cc:2085-2229) -----------------------
 * Every sequence of the batch tracks against the one map and graph of the handle.                                      */
#define FB_LOCAL_MAP_MAX_EXPAND 80 /* "if(mvpLocalKeyFrames.size()>80) break" (:2175)                                  */
typedef struct fb_local_map_args {
  int32_t batch, kp_stride;
  const int32_t *d_n;           /* [batch] mCurrentFrame.N                                                             */
  int32_t *d_map_point;         /* [batch][kp_stride] in/out: mvpMapPoints as indices into the map's points, -1 = NULL;
                                   an entry of a bad point becomes -1 (:2138)                                          */
  const uint8_t *d_kf_bad;      /* [max_keyframes] KeyFrame::isBad()                                                   */
  int32_t cap_kf;               /* a list never exceeds max(max_keyframes, 83) entries; more capacity is never used    */
  int32_t *d_local_kf;          /* [batch][cap_kf] in/out: mvpLocalKeyFrames                                           */
  int32_t *d_n_local_kf;        /* [batch] in/out                                                                      */
  int32_t cap_mp;
  int32_t *d_local_mp;          /* [batch][cap_mp] mvpLocalMapPoints                                                   */
  int32_t *d_n_local_mp;        /* [batch]                                                                             */
  int32_t *d_ref_kf;            /* [batch] in/out: mpReferenceKF, written only when there is a pKFmax (:2224-2228)     */
  int32_t *d_n_voters;          /* [batch] keyframeCounter.size(), bad key frames included                             */
  int32_t *d_overflow;          /* [batch] != 0: a list was longer than its capacity; what fitted is its prefix        */
  const int32_t *d_gate_row;    /* [batch] or NULL: a sequence with d_gate_row[b] < gate_min is left entirely alone    */
  int32_t gate_min;
  int32_t reuse_index;          /* 0: the point -> edge index is rebuilt from the edge list, like every other map call;
                                   1: the caller states that the last map-taking call on this handle used the same
                                   fb_covis_map arrays, unchanged, and its index (and kf_order ranks) are used again.
                                   A different map in that call is FB_ERR_ARG (pointers and sizes are compared; the
                                   contents are the caller's statement).  A host-pointer variant leaves no index: after
                                   one, or after the scratch had to grow, the index is rebuilt as with 0               */
} fb_local_map_args;
/* Votes (:2125-2141): every feature i < n with a point; a bad point (map.mp_bad) sets d_map_point[i] = -1 and does not
 * vote; otherwise every live edge of the point votes for its key frame (a point held at two features votes twice; edges
 * of bad key frames vote and are filtered later).  Empty counter (:2143-2144): d_local_kf, d_n_local_kf and d_ref_kf stay
 * as they came in, and UpdateLocalPoints runs on that list (read up to min(d_n_local_kf, cap_kf) entries).  Voters
 * (:2153-2168) in ascending kf_order, bad ones skipped; pKFmax is the first voter with a strictly larger count.
 * Expansion (:2172-2222) over the voters only, in order: size > 80 ends it; each step takes (a) the first of
 * GetBestCovisibilityKeyFrames(10) (bad ones occupy places) that is non-bad and unmarked, (b) the first child in set
 * order that is non-bad and unmarked, (c) the parent if it exists and is unmarked (no isBad test), which ends the whole
 * loop (the break at :2218 leaves the outer for).  Local points (:2095-2118): the local key frames in list order, the
 * features ascending, the first occurrence of every non-NULL, non-bad point; the key frame's own isBad is not tested.
 * A kf list the call builds is cut at cap_kf (the points come from what fitted), a point list at cap_mp; either sets
 * d_overflow.  A list that came in and is kept by an empty counter is NOT judged: if d_n_local_kf > cap_kf it is read up to
 * cap_kf, d_n_local_kf stays, and d_overflow reports the point list only.
 * Out-of-range entries (d_map_point >= n_mp, a carried-over key frame outside the slots) are skipped and counted.
 * Precondition: the frame is not the one with mnId == 0 (the initial marks equal it; Track never gets there).
 * Scratch: see fb_covis_reserve_local_map.                                                                             */
int fb_covis_local_map_dev(fb_covis *g, const fb_covis_map *map, const fb_local_map_args *a, void *stream);
int fb_covis_local_map(fb_covis *g, const fb_covis_map *map, const fb_local_map_args *a); /* host pointers throughout     */
/* Scratch for fb_covis_local_map_dev ahead of time.  The call keeps its own arrays BEHIND the index of the last
 * map-taking call ([that call's head][index][local map]), so a reused index is not overwritten, neither by this call nor
 * by the window's header arrays; n_q is the largest n_q of the fb_covis_update_connections_dev calls whose index is to be
 * reused, with_window != 0 sizes the head for a fb_covis_local_window_dev on the same map (front side).  If the scratch
 * has to grow, the index is lost and reuse_index = 1 rebuilds it once.                                                  */
int fb_covis_reserve_local_map(fb_covis *g, int32_t n_mp, int32_t n_obs, int32_t n_q, int32_t batch, int32_t with_window);

/* ---- the bird side of the graph: KeyFrame::UpdateBirdConnections (KeyFrame.cc:418-562) ---------------------------------
 * mvpBirdConnectedKeyFrames of every key frame, kept by the handle in the front rows' format (descending by (weight,
 * kf_order), derived on read); fb_covis_clear empties it, fb_covis_erase_keyframe_dev leaves it alone (SetBadFlag never
 * edits another key frame's bird list).  Of `map` only max_keyframes and kf_order are read; of `tables` kf_nb, kf_mpb,
 * mpb_bad and the bird edge list (one live edge per (point, key frame) pair, as for the front list).                    */
#define FB_COVIS_BIRD_TH 2        /* th of KeyFrame::UpdateBirdConnections (KeyFrame.cc:483); there is no pKFmax fallback */
/* UpdateBirdConnections(now_state) for the n_q key frames d_slots[0..n_q), with the result of calling them one after
 * another in list order (no other key frame's list is written, so the queries are independent).  Query q acts iff
 * d_n_counter[q] != 0 (the call that ends UpdateConnections, :701; d_n_counter is the output of the front call on the same
 * batch, NULL = every query acts) or now_state >= 3 (the empty-counter exit, :608-609); one that does not act writes
 * d_n_bird_counter[q] = 0 and d_bird_front[q] = the front of its unchanged list and nothing else.
 * Counter (:424-445): every feature i < kf_nb with a point that is not bad, every live bird edge of that point whose key
 * frame is not the slot itself; a point held at two features counts twice; the observer's isBad is not tested.
 * d_n_bird_counter[q] = KFcounter.size().
 * Empty counter (:447-480): the list stays; if now_state >= 3 and parent == -1 the nearest-earlier key frame becomes the
 * parent (:453-476): d_kf_in_map != 0, the largest frame id with 0 < id < this key frame's, the smaller kf_order among
 * equal ids (the rule of fb_covis_first_connection_dev); linked = 1, first = 0.  Where nothing qualifies the reference
 * dereferences an uninitialised pointer: nothing is done and the error counter goes up.
 * Otherwise (:483-559) the entries >= FB_COVIS_BIRD_TH, descending by (weight, kf_order), replace the list (also when there
 * are none); then, if parent == -1 or first != 0, and the slot is not id0_slot (mnId == 0, :516; -1 = none): parent = the
 * list's front when it has one, else the nearest-earlier key frame when now_state >= 3 (same rule); linked = 1, first = 0.
 * A slot whose parent is set while first != 0 gets the new parent in its place (the state holds one parent per slot).
 * d_bird_front[q] = mvpBirdConnectedKeyFrames.front() afterwards, -1 = empty.  d_kf_frame_id [max_keyframes] int32 and
 * d_kf_in_map [max_keyframes] uint8 may be NULL when now_state < 3.  mvOrderedWeights, which :512 overwrites with the bird
 * weights, is NOT touched: fb_covis_ordered / fb_covis_by_weight keep the front's weights.  Out-of-range entries and query
 * slots are skipped and counted.  Every call builds the bird edge index anew (the call keeps none), so an out-of-range
 * bird edge is counted once per CALL, not once per entry, like an out-of-range front edge by every front call that builds
 * its index; an out-of-range kf_mpb entry is counted once per acting query that walks it.  Scratch: behind the handle's index, see fb_covis_reserve_local_bird_map; the front
 * index a later reuse_index reads stays valid unless the scratch has to grow.  Enqueues only.                          */
int fb_covis_update_bird_connections_dev(fb_covis *g, const fb_covis_map *map, const fb_covis_kf_tables *tables, int32_t n_q,
                                         const int32_t *d_slots, const int32_t *d_n_counter, int32_t now_state,
                                         int32_t id0_slot, const int32_t *d_kf_frame_id, const uint8_t *d_kf_in_map,
                                         int32_t *d_n_bird_counter, int32_t *d_bird_front, void *stream);
int fb_covis_update_bird_connections(fb_covis *g, const fb_covis_map *map, const fb_covis_kf_tables *tables, int32_t n_q,
                                     const int32_t *slots, const int32_t *n_counter, int32_t now_state, int32_t id0_slot,
                                     const int32_t *kf_frame_id, const uint8_t *kf_in_map, int32_t *n_bird_counter,
                                     int32_t *bird_front); /* host pointers, the tables' arrays included */
/* GetBirdConnectedBirdKeyFrames() and the bird weights (d_weights may be NULL); arrays of max_keyframes entries, entries
 * past *d_n are left as they are                                                                                        */
int fb_covis_bird_connected_dev(fb_covis *g, int32_t slot, int32_t *d_n, int32_t *d_slots, int32_t *d_weights, void *stream);
int fb_covis_bird_connected(fb_covis *g, int32_t slot, int32_t *n, int32_t *slots, int32_t *weights);

/* ---- the local bird map: the bird block of Map::AddKeyFrame (Map.cc:41-46) and Map::UpdateLocalBirdMap (:97-153) ----------
 * The list after the push_front has new_slot at position 0.  Member j is near iff !(dis > 5) (:104-106), dis =
 * cv::norm(refTw - curTw, NORM_L2) of CV_32F: per component d = (double)(float)(ow[j] - ow[new]), dis = sqrt(d0 * d0 +
 * d1 * d1 + d2 * d2) in double, summed in that order.  The first holder of a bird point is the smallest position among the
 * near members that hold it in kf_mpb (only -1 is skipped; mpb_bad is not tested, :117); pMP_sum[j] = the distinct points
 * whose first holder is j; member j stays iff it is near and pMP_sum[j] >= 10 (:127), in the order it had.  The local
 * points are those held by ANY near member, the ones dropped for pMP_sum < 10 included (:120-128 inserts before the
 * test), in ascending d_mpb_order (the std::set's order).  Of `map` only max_keyframes is used; of `tables` kf_nb, kf_mpb,
 * n_mpb and, when d_kf_ow is NULL, kf_Tcw.                                                                                */
typedef struct fb_local_bird_map_args {
  int32_t new_slot;              /* pKF of AddKeyFrame: push_front, curTw = its camera centre (:43-44)                     */
  const float *d_kf_ow;          /* [max_keyframes][3] KeyFrame::GetCameraCenter() (:103); NULL: -Rcw^T tcw of
                                    tables->kf_Tcw, products and sum in double, as UpdateNormalAndDepth derives it         */
  const uint64_t *d_mpb_order;   /* [n_mpb] (uintptr_t)pMPB, the order of setlocalMapPointBirds (:99, :135); NULL: index   */
  int32_t cap_kf;                /* 1 .. max_keyframes                                                                     */
  int32_t *d_local_kf_bird;      /* [cap_kf] in/out: localKFbird, front first (:43, :108, :128)                            */
  int32_t *d_n_local_kf_bird;    /* [1] in/out                                                                             */
  int32_t cap_mpb;
  int32_t *d_local_mpb;          /* [cap_mpb] out: localMapPointBirds (:134-143) = fb_track_args.d_local_mpb               */
  int32_t *d_n_local_mpb;        /* [1] out, at most cap_mpb           = fb_track_args.d_n_local_mpb                       */
  int32_t *d_overflow;           /* [1] != 0: a result was longer than its capacity; what fitted is its prefix             */
} fb_local_bird_map_args;
/* An incoming list longer than cap_kf is read up to cap_kf; a member outside the slots is dropped and counted, as is a
 * kf_mpb entry >= n_mpb.  The `> 10` gate of Tracking::GetLocalMapForBird (Tracking.cc:2004) stays with the consumer
 * (fb_frame_track_dev).  The points are ranked among themselves by d_mpb_order: work quadratic in the local points, not
 * in the map.  Enqueues only.                                                                                           */
int fb_covis_local_bird_map_dev(fb_covis *g, const fb_covis_map *map, const fb_covis_kf_tables *tables,
                                const fb_local_bird_map_args *a, void *stream);
int fb_covis_local_bird_map(fb_covis *g, const fb_covis_map *map, const fb_covis_kf_tables *tables,
                            const fb_local_bird_map_args *a); /* host pointers throughout */
/* Scratch for the two bird calls ahead of time: a bird edge index of (n_mpb, n_bobs) and the local bird map's arrays,
 * BEHIND the index the handle holds at the time of the call (so call it after the front calls' reserve and first use; a
 * later growth loses that index once, as for fb_covis_reserve_local_map).  Also allocates the bird lists.               */
int fb_covis_reserve_local_bird_map(fb_covis *g, int32_t n_mpb, int32_t n_bobs);

/* ---- map correction: LoopClosing::CorrectLoop (LoopClosing.cc:438-541) and the map update that ends
 * LoopClosing::RunGlobalBundleAdjustment (:714-825), on fb_covis_map / fb_covis_kf_tables ---------------------------------
 * Neither call has a floating-point decision: every branch is NULL, bad, holder order or a flag.                        */
typedef struct fb_correct_loop_args {
  double q[4], t[3], s;         /* mg2oScw as g2o::Sim3's own members: r (x, y, z, w), t, s                            */
  int32_t cur_slot;             /* mpCurrentKF                                                                         */
  int32_t reuse_index;          /* as fb_local_map_args.reuse_index                                                    */
  const float *scale_factors;   /* [tables.n_levels] mvScaleFactors                                                    */
  const int32_t *mp_ref_kf;     /* [map.n_mp] mpRefKF as a slot                                                        */
  float *mp_normal;             /* [map.n_mp][3] in/out: mNormalVector                                                 */
  float *mp_min_dist;           /* [map.n_mp] in/out: mfMinDistance                                                    */
  float *mp_max_dist;           /* [map.n_mp] in/out: mfMaxDistance                                                    */
  int32_t *d_mp_corrected_ref;  /* [map.n_mp] mnCorrectedReference as a slot, -1: the point was not touched            */
  int32_t *d_n_set;             /* [1] mvpCurrentConnectedKFs.size()                                                   */
  int32_t *d_set_slots;         /* [max_keyframes] the set in ascending kf_order; entries past *d_n_set are left alone  */
  float *d_set_Scw;             /* [max_keyframes][12] or NULL: the corrected Sim3 of each set member, see below        */
} fb_correct_loop_args;
/* Precondition: the graph row of cur_slot is current (the reference calls UpdateConnections on it at :435; the caller
 * does that with fb_covis_update_connections_dev).  Reads of tables: kf_Tcw, n_levels, mp_xw and, unless kf_mpb is NULL
 * (no bird side), bird_stride, kf_nb, kf_mpb, n_mpb, mpb_bad, mpb_xw; nothing else of it is looked at.  The octave of
 * feature i is map.kf_octave.
 * Set (:438-439) = GetVectorCovisibleKeyFrames(cur) followed by cur, bad key frames included (no isBad test).
 * NonCorrectedSim3[i] = Sim3(Riw, tiw, 1); CorrectedSim3[i] = Sim3(Ric, tic, 1) * Scw with Tic = Tiw * Twc(cur), a CV_32F
 * product; CorrectedSim3[cur] = Scw; all from the poses as they come in.  Twc and Ow of a pose are what
 * KeyFrame::SetPose makes of it (KeyFrame.cc:104-118); cv::Mat products accumulate in double and round once; the Sim3
 * algebra is g2o's (sim3.h:64, :144, :233, :266) in double.
 * Map points: the point loop iterates a std::map<KeyFrame*, Sim3>, so it runs in ascending kf_order, not in list order.
 * A non-NULL, non-bad point is moved once, by the holder with the smallest kf_order among the set members whose kf_mp row
 * contains it (mnCorrectedByKF), through CorrectedSwi.map(Siw.map(P)) of that holder; d_mp_corrected_ref = that slot.
 * UpdateNormalAndDepth (MapPoint.cc:330-371) runs on each moved point inside that serial loop, so it sees a half-corrected
 * map: each observer (live edge; bad key frames are not tested) contributes its camera centre, an observer that is in the
 * set with kf_order strictly smaller than the holder's its CORRECTED centre, every other observer its old one -- the
 * holder itself included, whose SetPose comes after its point loop.  dist is to the reference key frame's centre under
 * the same rule; level is the octave at observations[pRefKF], and when the reference key frame is not among the observers
 * operator[] inserts 0 there, so the level is feature 0's octave.  A point with no live edge keeps its normal and
 * distances; it is still moved.  mfMaxDistance = dist * scale[level], mfMinDistance = max / scale[n_levels - 1],
 * normal / n.
 * Bird points (:506-525): line :523 is a comparison, not an assignment, so a bird point is never marked.  Every set
 * member that holds it in kf_mpb moves it again (once per feature it is held at), in ascending kf_order, each applying
 * its own CorrectedSwi o Siw to the result of the one before.
 * Poses: kf_Tcw[i] = [R(CorrectedSiw) | t / s] for every set member, written after all reads of old poses.
 * d_set_slots is the list to hand to fb_covis_update_connections_dev for the UpdateConnections at :540: those calls
 * depend on no pose, so one batched call after this one equals the interleaved calls.
 * Out-of-range entries (kf_mp, kf_mpb, and for a moved point with a live edge mp_ref_kf and the octave, which then keeps
 * its normal and distances) are skipped and counted (fb_covis_error_count), never used as an index.
 * d_set_Scw, when not NULL: row k = rows 0..2 of Converter::toCvMat(CorrectedSim3[d_set_slots[k]]), s * R and t of the
 * double Sim3, each cast to float once: the Scw that SearchAndFuse projects with.  It cannot be recovered afterwards (the
 * poses are overwritten and hold [R | t / s] rounded).  NULL: not written, nothing else changes.
 * Not restated: OptimizeEssentialGraph; the loop fusion (:545-560) is fb_covis_loop_fuse_dev, SearchAndFuse
 * fb_covis_search_and_fuse_dev, LoopConnections (:571-589) fb_covis_loop_connections_dev.  Enqueues only.               */
int fb_covis_correct_loop_dev(fb_covis *g, const fb_covis_map *map, const fb_covis_kf_tables *tables,
                              const fb_correct_loop_args *a, void *stream);
int fb_covis_correct_loop(fb_covis *g, const fb_covis_map *map, const fb_covis_kf_tables *tables,
                          const fb_correct_loop_args *a); /* host pointers throughout */
/* Scratch for fb_covis_correct_loop_dev ahead of time: behind the index, like fb_covis_reserve_local_map; n_mpb and
 * bird_stride are 0 without the bird side (which takes max_keyframes * bird_stride ints).                              */
int fb_covis_reserve_correct_loop(fb_covis *g, int32_t n_mp, int32_t n_obs, int32_t n_q, int32_t n_mpb, int32_t bird_stride);

typedef struct fb_propagate_gba_args {
  int32_t n_origins;
  const int32_t *origins;       /* [n_origins] mvpKeyFrameOrigins as slots                                             */
  uint8_t *kf_gba;              /* [max_keyframes] in/out: mnBAGlobalForKF == nLoopKF                                  */
  float *kf_Tcw_gba;            /* [max_keyframes][12] in/out: mTcwGBA                                                 */
  float *kf_Tcw_bef;            /* [max_keyframes][12] in/out: mTcwBefGBA                                              */
  const uint8_t *mp_gba;        /* [map.n_mp] mnBAGlobalForKF == nLoopKF of the point                                  */
  const float *mp_pos_gba;      /* [map.n_mp][3] mPosGBA                                                               */
  const int32_t *mp_ref_kf;     /* [map.n_mp] mpRefKF as a slot                                                        */
  const uint8_t *mpb_gba;       /* [tables.n_mpb] } the same for MapPointBird; mpb_ref_kf == -1: pRefKF == NULL        */
  const float *mpb_pos_gba;     /* [tables.n_mpb][3] }                                                                 */
  const int32_t *mpb_ref_kf;    /* [tables.n_mpb] }                                                                    */
  uint8_t *d_reached;           /* [max_keyframes] 1: the walk visited the key frame                                   */
} fb_propagate_gba_args;
/* Reads of tables: kf_Tcw, mp_xw and, unless mpb_xw is NULL (no bird side), n_mpb, mpb_bad, mpb_xw; of map: n_mp, mp_bad.
 * Key frames (:715-740): a breadth-first walk from the origins over GetChilds(), which is parent[c] == a && linked[c] of
 * the handle's tree.  For an unflagged child TcwGBA = (Tcw_child * Twc_parent) * TcwGBA_parent, two CV_32F 4x4 products,
 * each rounded, and its flag is set.  Both factors of the first product are OLD poses: Twc is read at :721 before the
 * parent's SetPose at :737; the only dependence on the walk is through the parent's TcwGBA.  Every visited key frame
 * gets kf_Tcw_bef = kf_Tcw and then kf_Tcw = kf_Tcw_gba.  Key frames that are not reached keep all three arrays.
 * Precondition, checked and counted rather than trusted: the origins are distinct slots with parent == -1; an entry that
 * is out of range, has a parent, or repeats an earlier one is counted and left out.  The walk then ends on any input; one
 * deeper than max_keyframes levels would stop and be counted.
 * Points (:747-825), after the key frames: a bad point is left alone; a flagged point becomes its pos_gba; otherwise the
 * point is skipped unless its reference key frame's flag is set after the walk, and then becomes
 * Rwc * (Rcw_bef * P + tcw_bef) + twc, with Rcw_bef / tcw_bef from kf_Tcw_bef as it stands (for a flagged but unreached
 * key frame that is whatever the caller passed, which is why the array is in/out) and Twc that of the new pose.  A map
 * point whose reference is -1 or out of range is skipped and counted (the reference dereferences it); a bird point
 * whose reference is -1 is skipped (:799-803), out of range skipped and counted.  Enqueues only; no scratch.            */
int fb_covis_propagate_gba_dev(fb_covis *g, const fb_covis_map *map, const fb_covis_kf_tables *tables,
                               const fb_propagate_gba_args *a, void *stream);
int fb_covis_propagate_gba(fb_covis *g, const fb_covis_map *map, const fb_covis_kf_tables *tables,
                           const fb_propagate_gba_args *a); /* host pointers throughout */

/* ---- the per-point side of LocalMapping: MapPoint::UpdateNormalAndDepth / ComputeDistinctiveDescriptors
 * (MapPoint.cc:242-307, :330-371), LocalMapping::ProcessNewKeyFrame (LocalMapping.cc:158-179) and MapPointCulling
 * (:207-228) on fb_covis_map.  These are the calls in which the library writes the caller's map arrays: each names the
 * arrays it writes, and the writable pointers of the last two must be the map's own.                                   */
#define FB_REFRESH_NORMAL_DEPTH 1
#define FB_REFRESH_DESCRIPTOR 2
#define FB_REFRESH_STAGE 128 /* observers whose descriptors one wave stages in LDS; a longer list reads kf_desc          */
typedef struct fb_point_refresh_args {
  const int32_t *d_list;        /* [n_list] map point indices, or NULL: every point of the map (n_list, d_n_list ignored) */
  const int32_t *d_n_list;      /* [1] the list's length on the device (clamped to n_list), or NULL: n_list              */
  int32_t n_list;               /* the list's length, or its capacity when d_n_list is given                           */
  int32_t what;                 /* FB_REFRESH_NORMAL_DEPTH | FB_REFRESH_DESCRIPTOR                                       */
  int32_t reuse_index;          /* as fb_local_map_args.reuse_index                                                    */
  int32_t n_levels;             /* 1 .. FB_MAX_LEVELS                                                                  */
  const float *kf_Tcw;          /* [max_keyframes][12]                                                                 */
  const uint8_t *kf_bad;        /* [max_keyframes] KeyFrame::isBad()                                                   */
  const uint8_t *kf_desc;       /* [max_keyframes][kp_stride][32] mDescriptors; 16-byte aligned                        */
  const float *scale_factors;   /* [n_levels] mvScaleFactors                                                           */
  const float *mp_xw;           /* [map.n_mp][3]                                                                       */
  const int32_t *mp_ref_kf;     /* [map.n_mp] mpRefKF as a slot                                                        */
  float *mp_normal;             /* [map.n_mp][3] in/out                                                                */
  float *mp_min_dist;           /* [map.n_mp] in/out                                                                   */
  float *mp_max_dist;           /* [map.n_mp] in/out                                                                   */
  uint8_t *mp_desc;             /* [map.n_mp][32] in/out: mDescriptor; 16-byte aligned                                 */
} fb_point_refresh_args;
/* For every listed point, one wave.  A bad point and a point without a live edge keep everything.  The observers are the
 * point's live edges in ascending kf_order (the reference iterates a std::map<KeyFrame*, size_t>).
 * Normal and depth: every observer contributes, bad key frames included (no isBad test at :350-357); the CV_32F sum of
 * unit vectors runs in observer order, each norm accumulated in double; Ow is what KeyFrame::SetPose makes of kf_Tcw; dist
 * is to the reference key frame's centre; level is the octave at observations[pRefKF], feature 0's when the reference key
 * frame is no observer (operator[] inserts 0); mfMaxDistance = dist * scale[level], mfMinDistance = max / scale[n_levels -
 * 1], normal / n.  A reference slot or a level out of range is counted and the point keeps its normal and distances.
 * Descriptor: the observers whose key frame is not bad (:265); none: the descriptor stays.  The observer with the least
 * median distance (index (int)(0.5 * (N - 1)) of its sorted row), the first in observer order among equals, gives its 32
 * bytes.  Any number of observers up to max_keyframes is handled; up to FB_REFRESH_STAGE descriptors are staged in LDS.
 * A point listed twice gives what listing it once gives.  A list entry outside [0, n_mp) is skipped and counted.  The
 * point -> edge index is built or reused like in fb_covis_correct_loop_dev and stays valid.  Enqueues only.            */
int fb_covis_refresh_points_dev(fb_covis *g, const fb_covis_map *map, const fb_point_refresh_args *a, void *stream);
int fb_covis_refresh_points(fb_covis *g, const fb_covis_map *map, const fb_point_refresh_args *a); /* host pointers; d_n_list
                                                                                                      must be NULL           */
int fb_covis_reserve_refresh_points(fb_covis *g, int32_t n_mp, int32_t n_obs, int32_t n_q);

typedef struct fb_new_keyframe_args {
  int32_t slot;                 /* mpCurrentKeyFrame; kf_n, kf_mp, kf_octave, kf_desc and its pose are filled already   */
  int32_t n_features;           /* its N as the host knows it; 0 .. kp_stride                                          */
  int32_t obs_cap;              /* capacity of the edge arrays; map.n_obs + n_features <= obs_cap                      */
  int32_t *obs_mp, *obs_kf, *obs_idx;  /* the map's edge arrays, writable (the same pointers as in map)               */
  int32_t *d_n_added;           /* [1] the number of new edges                                                         */
  int32_t recent_cap;
  int32_t *d_recent;            /* [recent_cap] in/out: mlpRecentAddedMapPoints as point indices                       */
  int32_t *d_n_recent;          /* [1] in/out                                                                          */
  fb_point_refresh_args refresh; /* the arrays of the refresh; d_list, d_n_list, n_list, what, reuse_index are ignored  */
} fb_new_keyframe_args;
/* For i = 0 .. n_features - 1 in order: a NULL entry and a bad point are skipped; a point with no live edge to slot gets
 * the edge (mp, slot, i) and is refreshed, both parts, on the grown edge list; a point that has one (an edge added earlier
 * in this loop included: a point held at two features, at its second) is appended to d_recent, in ascending i.  An entry
 * that does not fit recent_cap is dropped and counted.
 * The call owns the block [map.n_obs, map.n_obs + n_features) of the edge arrays: the new edges first, in ascending i, the
 * rest tombstones (obs_kf = obs_mp = obs_idx = -1).  Without waiting, the caller goes on with n_obs + n_features, and may
 * compact later.  If kf_n[slot] != n_features the block is all tombstones, *d_n_added = 0, nothing else is written and one
 * error is counted.  UpdateConnections and the mbFirstConnection block stay fb_covis_update_connections_dev and
 * fb_covis_first_connection_dev on the grown map.  The handle's index is invalid afterwards.  Enqueues only.            */
int fb_covis_process_new_keyframe_dev(fb_covis *g, const fb_covis_map *map, const fb_new_keyframe_args *a, void *stream);
int fb_covis_process_new_keyframe(fb_covis *g, const fb_covis_map *map, const fb_new_keyframe_args *a); /* host pointers */
int fb_covis_reserve_process_new_keyframe(fb_covis *g, int32_t n_mp, int32_t n_obs, int32_t n_q, int32_t n_features);

typedef struct fb_map_point_culling_args {
  int32_t cur_kf_id;            /* (int)mpCurrentKeyFrame->mnId                                                        */
  int32_t n_th_obs;             /* 2 monocular, 3 otherwise (:200-205)                                                 */
  const int32_t *mp_first_kf_id; /* [map.n_mp] (int)mnFirstKFid; -1 for a point made from a Frame                      */
  const int32_t *mp_found;      /* [map.n_mp] mnFound                                                                  */
  const int32_t *mp_visible;    /* [map.n_mp] mnVisible                                                                */
  int32_t recent_cap;
  int32_t *d_recent;            /* [recent_cap] in/out; the kept entries stay in list order                            */
  int32_t *d_n_recent;          /* [1] in/out (read clamped to recent_cap)                                             */
  int32_t *kf_mp;               /* } the map's arrays, writable (the same pointers as in map)                          */
  uint8_t *mp_bad;              /* }                                                                                   */
  int32_t *obs_kf;              /* }                                                                                   */
  int32_t *d_n_culled;          /* [1]                                                                                 */
  int32_t *d_culled;            /* [recent_cap] the points that got SetBadFlag, in list order (for Map::EraseMapPoint) */
  int32_t *d_n_erased;          /* [1] rows wanted; rows past erased_cap are not written                               */
  int32_t erased_cap;
  int32_t *d_erased;            /* [erased_cap][4] the erased edges as rows (key frame slot, point index, feature index,
                                   edge index), the row shape of fb_covis_window_scatter_dev: grouped by point in the
                                   order of d_culled, within a point in ascending kf_order                              */
} fb_map_point_culling_args;
/* The walk of :207-228 over the list, in the reference's branch order: a bad point is dropped; (float)found / visible <
 * 0.25f (the int -> float conversions and one correctly rounded division as written: visible == 0 gives inf or NaN, and a
 * comparison with NaN is false) -> SetBadFlag, dropped; cur - first >= 2 && Observations() <= n_th_obs -> SetBadFlag,
 * dropped; cur - first >= 3 -> dropped; otherwise kept.  Observations() is the number of live edges.  SetBadFlag
 * (MapPoint.cc:151-168): mp_bad = 1, every live edge of the point becomes a tombstone (obs_kf = -1) and kf_mp[kf][idx] = -1
 * for each, unconditionally like EraseMapPointMatch(idx).  A point listed twice takes its branch at the first entry and is
 * dropped as bad at the second, as in the serial walk.  A list entry outside [0, n_mp) is dropped and counted.  The graph
 * is not touched.  The handle's index is invalid afterwards.  Enqueues only.                                           */
int fb_covis_map_point_culling_dev(fb_covis *g, const fb_covis_map *map, const fb_map_point_culling_args *a, void *stream);
int fb_covis_map_point_culling(fb_covis *g, const fb_covis_map *map, const fb_map_point_culling_args *a); /* host pointers */
int fb_covis_reserve_map_point_culling(fb_covis *g, int32_t n_mp, int32_t n_obs, int32_t n_q, int32_t recent_cap);

/* ---- MapPoint::Replace (MapPoint.cc:177-215) and the loop fusion of LoopClosing::CorrectLoop (LoopClosing.cc:545-560) on
 * fb_covis_map.  Integer and byte work throughout; the descriptor is the rule of fb_covis_refresh_points.               */
typedef struct fb_point_fuse_arrays {
  int32_t *kf_mp;               /* } the map's arrays, writable (the same pointers as in map)                          */
  uint8_t *mp_bad;              /* }                                                                                   */
  int32_t *obs_mp, *obs_kf;     /* }                                                                                   */
  int32_t *mp_found;            /* [map.n_mp] in/out: mnFound                                                          */
  int32_t *mp_visible;          /* [map.n_mp] in/out: mnVisible                                                        */
  int32_t *mp_replaced;         /* [map.n_mp] in/out: mpReplaced as a point index, -1 = NULL                           */
  const uint8_t *kf_bad;        /* [max_keyframes] KeyFrame::isBad()                                                   */
  const uint8_t *kf_desc;       /* [max_keyframes][kp_stride][32] mDescriptors; 16-byte aligned                        */
  uint8_t *mp_desc;             /* [map.n_mp][32] in/out: mDescriptor; 16-byte aligned                                 */
  int32_t *d_n_replaced;        /* [1] rows wanted; rows past replaced_cap are not written                             */
  int32_t replaced_cap;
  int32_t *d_replaced;          /* [replaced_cap][2] the (from, to) pairs that took effect, in execution order (for
                                   Map::EraseMapPoint and the host's objects)                                          */
} fb_point_fuse_arrays;

typedef struct fb_replace_points_args {
  int32_t n_pairs;              /* the list's length, or its capacity when d_n_pairs is given                          */
  const int32_t *d_n_pairs;     /* [1] the length on the device (clamped to n_pairs), or NULL                          */
  const int32_t *d_from, *d_to; /* [n_pairs] from[i]->Replace(to[i]); from[i] < 0: skipped (a NULL of vpReplacePoints)  */
  fb_point_fuse_arrays map;
} fb_replace_points_args;
/* The pairs applied one after another in list order, each exactly as MapPoint.cc:177-215.  from == to: nothing (mnId
 * equality is index equality).  Otherwise the live edges of `from` are taken; mp_bad[from] = 1, mp_replaced[from] = to; for
 * each taken edge (kf, idx): if `to` has no live edge to kf (IsInKeyFrame is decided by edges, not by kf_mp), kf_mp[kf][idx]
 * = to and the edge becomes to's (obs_mp[e] = to in place), else kf_mp[kf][idx] = -1 and the edge becomes a tombstone
 * (obs_kf[e] = -1); then found[to] += found[from], visible[to] += visible[from], and ComputeDistinctiveDescriptors(to) on
 * the edited map at that moment, with the rule of fb_covis_refresh_points (a bad `to` and a `to` without a live edge keep
 * their descriptor).  Neither point is tested for isBad: a `from` that an earlier pair replaced has no edges left, is
 * marked again (mp_replaced takes the later `to`), adds its found / visible a second time and refreshes the second `to`.
 * UpdateNormalAndDepth is not called: normal and distances stay.  The order in which one pair's edges are taken does not
 * show, by the precondition that a (mp, kf) pair occurs once among the live edges.  A pair with an index outside [0, n_mp)
 * (from < 0 apart) is skipped and counted, as is a pair one of whose points has more live edges than max_keyframes.
 * The overflow contract (a repeated (mp, kf) edge broke the precondition), for the three calls of this section: such a
 * pair is skipped whole -- no entry of the map, of the per-point arrays or of d_replaced is written, d_n_replaced does not
 * count it -- one error is counted, and the pairs after it run.  Where the loop fusion or step 3 of
 * fb_covis_search_and_fuse meets such a point at an empty feature, the step is AddObservation's early return plus one
 * error: kf_mp[kf][feature] = the point is written (and counts in nFused), no edge is made, no row of d_added, no
 * descriptor refresh; the features after it run.  Exactly max_keyframes live edges is no overflow.
 * One wave walks the list; the cost is the sum of the edges of the points named, not n_pairs * n_obs.  The handle's
 * index is invalid afterwards.  Enqueues only.                                                                         */
int fb_covis_replace_points_dev(fb_covis *g, const fb_covis_map *map, const fb_replace_points_args *a, void *stream);
int fb_covis_replace_points(fb_covis *g, const fb_covis_map *map, const fb_replace_points_args *a); /* host pointers; d_n_pairs
                                                                                                       must be NULL          */
int fb_covis_reserve_replace_points(fb_covis *g, int32_t n_mp, int32_t n_obs, int32_t n_q);

typedef struct fb_loop_fuse_args {
  int32_t cur_slot;             /* mpCurrentKF                                                                         */
  int32_t n_features;           /* its N as the host knows it (mvpCurrentMatchedPoints.size()); 0 .. kp_stride         */
  const int32_t *d_matched;     /* [n_features] mvpCurrentMatchedPoints as point indices, -1 = NULL                    */
  int32_t obs_cap;              /* capacity of the edge arrays; map.n_obs + n_features <= obs_cap (FB_ERR_CAPACITY)    */
  int32_t *obs_idx;             /* the map's obs_idx, writable (the same pointer as in map)                            */
  int32_t *d_n_added;           /* [1] the number of new edges                                                         */
  int32_t added_cap;
  int32_t *d_added;             /* [added_cap][4] the new edges as rows (key frame slot, point, feature, edge)         */
  fb_point_fuse_arrays map;
} fb_loop_fuse_args;
/* For i = 0 .. n_features - 1 in order with matched[i] >= 0: if kf_mp[cur][i] >= 0 as it stands at that moment, it is
 * Replace(kf_mp[cur][i] -> matched[i]) as above; else kf_mp[cur][i] = matched[i], AddObservation(matched[i], cur, i), which
 * returns early when the point has a live edge to cur already (MapPoint.cc:101: kf_mp is written, no edge is), and
 * ComputeDistinctiveDescriptors(matched[i]).  The same loop point at two features follows from that.
 * The call owns the block [map.n_obs, map.n_obs + n_features) of the edge arrays, as fb_covis_process_new_keyframe_dev does:
 * the new edges first, in ascending i, the rest tombstones; the caller goes on with n_obs + n_features.  If kf_n[cur] !=
 * n_features the block is all tombstones, both counts are 0, nothing else is written and one error is counted.  An entry of
 * matched or of kf_mp[cur] >= n_mp is skipped and counted.  The handle's index is invalid afterwards.  Enqueues only.    */
int fb_covis_loop_fuse_dev(fb_covis *g, const fb_covis_map *map, const fb_loop_fuse_args *a, void *stream);
int fb_covis_loop_fuse(fb_covis *g, const fb_covis_map *map, const fb_loop_fuse_args *a); /* host pointers */
int fb_covis_reserve_loop_fuse(fb_covis *g, int32_t n_mp, int32_t n_obs, int32_t n_q, int32_t n_features);

/* LoopClosing::SearchAndFuse (LoopClosing.cc:616-642) with ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)
 * (ORBmatcher.cc:978-1101) on fb_covis_map.                                                                             */
typedef struct fb_search_and_fuse_args {
  int32_t n_set;                /* key frames (a launch parameter, as for the batched UpdateConnections); 0 .. max_keyframes */
  const int32_t *d_set_slots;   /* [n_set] processed in the order given (fb_covis_correct_loop writes ascending kf_order,
                                   the order of the reference's std::map<KeyFrame*, g2o::Sim3>)                        */
  const float *d_set_Scw;       /* [n_set][12] rows 0..2 of Converter::toCvMat(CorrectedSim3[slot])                    */
  int32_t n_loop;
  const int32_t *d_loop_mp;     /* [n_loop] mvpLoopMapPoints as point indices                                          */
  float th;                     /* 4 at LoopClosing.cc:628; TH_LOW is the matcher's constant                           */
  fb_camera cam;                /* } the key-frame side that is the same for every key frame, as in fb_kf_target       */
  fb_grid_geom grid;            /* }                                                                                   */
  float scale_factors[FB_MAX_LEVELS];
  float inv_level_sigma2[FB_MAX_LEVELS];
  float log_scale_factor;
  int32_t n_levels;
  const fb_keypoint *kf_keys_un; /* [max_keyframes][kp_stride] mvKeysUn by slot                                        */
  const float *mp_xw;           /* [map.n_mp][3] } the MapPoint getters of the search                                  */
  const float *mp_normal;       /* [map.n_mp][3] }                                                                     */
  const float *mp_min_dist;     /* [map.n_mp]    }                                                                     */
  const float *mp_max_dist;     /* [map.n_mp]    }                                                                     */
  int32_t obs_cap;              /* capacity of the edge arrays; map.n_obs + n_set * kp_stride <= obs_cap (FB_ERR_CAPACITY) */
  int32_t *obs_idx;             /* the map's obs_idx, writable (the same pointer as in map)                            */
  int32_t *d_n_fused;           /* [n_set] nFused of each Fuse                                                         */
  int32_t *d_n_added;           /* [1] new edges of the whole call                                                     */
  int32_t added_cap;
  int32_t *d_added;             /* [added_cap][4] rows (key frame slot, point, feature, edge) in execution order       */
  fb_point_fuse_arrays map;     /* d_replaced: the pairs of the whole call in execution order                          */
} fb_search_and_fuse_args;
/* Per key frame k, in order, on the map as the key frame before left it:
 *  1. valid[i] = !bad(loop[i]) && loop[i] is not among the non-bad entries of kf_mp[slot] (spAlreadyFound, taken once, :994);
 *  2. fb_fuse_sim3_search_dev with batch = 1 on the descriptors and bad flags as they stand; the key frame's grid is built
 *     by the call in scratch from kf_keys_un, the caller keeps none;
 *  3. the commit, serial in i (:1083-1097), for best[i] >= 0: p = kf_mp[slot][best] as it stands, adds made earlier in this
 *     loop included; p >= 0: rep[i] = p if p is not bad, else nothing; p < 0: AddObservation(loop[i], slot, best) with its
 *     early return, and kf_mp[slot][best] = loop[i]; each counts in nFused.  Two loop points that win the same empty feature:
 *     the first adds, the second gets rep = the first;
 *  4. Replace(rep[i] -> loop[i]) for i ascending with rep[i] >= 0 (:633-640), as fb_covis_replace_points_dev.
 * New edges: key frame k owns [map.n_obs + k * kp_stride, map.n_obs + (k + 1) * kp_stride) of the edge arrays, its new
 * edges first in the order they were made, the rest tombstones; the caller goes on with n_obs + n_set * kp_stride.
 * A slot, a loop point or a kf_mp entry out of range is skipped and counted.  No host wait between key frames: four
 * launches each on one stream.  The handle's index is invalid afterwards.  Enqueues only.                              */
int fb_covis_search_and_fuse_dev(fb_covis *g, const fb_covis_map *map, const fb_search_and_fuse_args *a, void *stream);
int fb_covis_search_and_fuse(fb_covis *g, const fb_covis_map *map, const fb_search_and_fuse_args *a); /* host pointers */
int fb_covis_reserve_search_and_fuse(fb_covis *g, int32_t n_mp, int32_t n_obs, int32_t n_q, int32_t kp_stride, int32_t n_set,
                                     int32_t n_loop, int32_t grid_cells);

/* ---- LocalMapping::SearchInNeighbors (LocalMapping.cc:478-558) with ORBmatcher::Fuse(pKF, vpMapPoints, th)
 * (ORBmatcher.cc:826-976) on fb_covis_map, in two calls: the target list from the handle's graph, then everything else. */
#define FB_FUSE_TARGETS_MAX 4096 /* entries of a target list that fb_covis_search_in_neighbors reads                     */
/* The target list of :481-503 for the key frame in cur_slot: for each of GetBestCovisibilityKeyFrames(nn) of cur_slot that
 * is not bad, the key frame is pushed and stamped, then each of its GetBestCovisibilityKeyFrames(nn2) is pushed if it is
 * not bad, not stamped and not cur_slot.  Second neighbours are pushed without being stamped, as in the reference: a key
 * frame reached through two first neighbours is listed twice, and again when its own turn as a first neighbour comes; a
 * second neighbour that is an earlier first neighbour is skipped.  The stamps are this call's (mnFuseTargetForKF of another
 * key frame's call cannot equal cur's id).  d_targets[target_cap] holds the list in that order, *d_n_targets its uncut
 * length; if that exceeds target_cap what fits is written and one error is counted (fb_covis_error_count).
 * nn * (1 + nn2) always suffices.  nn = 20 (monocular) and nn2 = 5 at :483, :495.  Enqueues only.                          */
int fb_covis_fuse_targets_dev(fb_covis *g, int32_t cur_slot, int32_t nn, int32_t nn2, const uint8_t *d_kf_bad /* [max_keyframes] */,
                              int32_t target_cap, int32_t *d_n_targets, int32_t *d_targets, void *stream);
int fb_covis_fuse_targets(fb_covis *g, int32_t cur_slot, int32_t nn, int32_t nn2, const uint8_t *kf_bad, int32_t target_cap,
                          int32_t *n_targets, int32_t *targets); /* host pointers */

typedef struct fb_search_in_neighbors_args {
  int32_t cur_slot;             /* mpCurrentKeyFrame                                                                   */
  int32_t n_features;           /* its N as the host knows it; 0 .. kp_stride                                          */
  int32_t n_targets;            /* launches of step 2 (a launch parameter); 0 .. FB_FUSE_TARGETS_MAX.  The exact count
                                   read once from d_n_targets, or the cap: a launch past *d_n_targets returns at once   */
  const int32_t *d_n_targets;   /* [1] } as fb_covis_fuse_targets_dev left them (the count is clamped to n_targets)      */
  const int32_t *d_targets;     /* [n_targets] }                                                                       */
  float th;                     /* 3, the default of Fuse at LocalMapping.cc:513, :538                                 */
  fb_camera cam;                /* } the key-frame side that is the same for every key frame, as in fb_kf_target       */
  fb_grid_geom grid;            /* }                                                                                   */
  float scale_factors[FB_MAX_LEVELS];
  float inv_level_sigma2[FB_MAX_LEVELS];
  float log_scale_factor;
  int32_t n_levels;
  const fb_keypoint *kf_keys_un; /* [max_keyframes][kp_stride] mvKeysUn by slot                                        */
  const float *kf_Tcw;          /* [max_keyframes][12]; Rcw|tcw of the search, and Ow as KeyFrame::SetPose makes it    */
  const float *mp_xw;           /* [map.n_mp][3]                                                                       */
  float *mp_normal;             /* [map.n_mp][3] } read by the search, written by step 5                               */
  float *mp_min_dist;           /* [map.n_mp]    }                                                                     */
  float *mp_max_dist;           /* [map.n_mp]    }                                                                     */
  const int32_t *mp_ref_kf;     /* [map.n_mp] mpRefKF as a slot                                                        */
  int32_t obs_cap;              /* capacity of the edge arrays; map.n_obs + new_edge_cap <= obs_cap (FB_ERR_CAPACITY)  */
  int32_t *obs_idx;             /* the map's obs_idx, writable (the same pointer as in map)                            */
  int32_t new_edge_cap;         /* edges the whole call may add                                                        */
  int32_t *d_n_fused;           /* [n_targets + 1] nFused of each Fuse of step 2 (0 for an idle launch); the last is step 4's */
  int32_t cand_cap;
  int32_t *d_n_candidates;      /* [1] vpFuseCandidates.size(), uncut                                                  */
  int32_t *d_candidates;        /* [cand_cap] vpFuseCandidates as point indices                                        */
  int32_t *d_n_added;           /* [1] new edges of the whole call                                                     */
  int32_t added_cap;
  int32_t *d_added;             /* [added_cap][4] rows (key frame slot, point, feature, edge) in execution order       */
  int32_t *d_n_counter;         /* [1] } of the closing UpdateConnections of cur_slot, as fb_covis_update_connections_dev */
  int32_t *d_front;             /* [1] }                                                                               */
  fb_point_fuse_arrays map;     /* d_replaced: the pairs of the whole call in execution order                          */
} fb_search_in_neighbors_args;
/* On one stream, without a host wait:
 *  2. vpMapPointMatches = kf_mp[cur][0 .. n_features) is copied once.  Then per target k < *d_n_targets, in list order
 *     (duplicates included), on the map as the target before left it: valid[i] = the snapshot's entry is not NULL, not bad
 *     and has no live edge to the target (IsInKeyFrame is decided by edges); fb_fuse_search_dev with batch = 1 on the
 *     descriptors, normals and distances as they stand, the pose and centre from kf_Tcw[target]; the commit (:952-972),
 *     serial in i for best[i] >= 0, with valid[i] decided again on the live map: p = kf_mp[target][best] as it stands;
 *     p >= 0 and not bad: Observations(p) > Observations(pMP) gives pMP->Replace(p), else p->Replace(pMP), both as
 *     fb_covis_replace_points_dev (Observations = live edges; equality replaces p); p >= 0 and bad: nothing; p < 0:
 *     AddObservation(pMP, target, best) and kf_mp[target][best] = pMP, without a descriptor refresh.  Each of the three
 *     counts in nFused.
 *  3. vpFuseCandidates: over the targets in list order, features ascending, every entry that is not NULL and not bad, at its
 *     first occurrence, on the map as step 2 left it.  If the count exceeds cand_cap the first cand_cap are kept and fused,
 *     and one error is counted.
 *  4. the same Fuse with the key frame cur_slot and the candidates; its nFused is d_n_fused[n_targets].
 *  5. every point that kf_mp[cur][0 .. n_features) holds now, if it is not bad: ComputeDistinctiveDescriptors and
 *     UpdateNormalAndDepth as fb_covis_refresh_points_dev (mp_normal, mp_min_dist, mp_max_dist, map.mp_desc are written).
 *  6. UpdateConnections of cur_slot as fb_covis_update_connections_dev with n_q = 1.  UpdateBirdConnections and
 *     fb_covis_first_connection_dev stay the caller's follow-up calls, as after every other UpdateConnections.
 * New edges: the call owns the block [map.n_obs, map.n_obs + new_edge_cap) of the edge arrays: its new edges in the order
 * they were made, the rest tombstones; the caller goes on with n_obs + new_edge_cap.  An add that finds the block full is
 * not made at all (no kf_mp write, no edge, not counted in nFused); one error is counted and the steps after it run.
 * If kf_n[cur] != n_features the block is all tombstones, every count is 0, *d_front = -1, nothing else is written and one
 * error is counted.  A target slot, a snapshot entry, a candidate or a kf_mp entry out of range is skipped and counted
 * (a snapshot entry once per target).  The overflow contract of fb_covis_replace_points holds.  Afterwards the handle's
 * point -> edge index is the one of the grown map (n_obs + new_edge_cap) and is valid for a reuse_index.  The scratch is
 * sized by fb_covis_reserve_search_in_neighbors or by the call.  Enqueues only: 4 launches per target and per step 4.      */
int fb_covis_search_in_neighbors_dev(fb_covis *g, const fb_covis_map *map, const fb_search_in_neighbors_args *a, void *stream);
int fb_covis_search_in_neighbors(fb_covis *g, const fb_covis_map *map, const fb_search_in_neighbors_args *a); /* host pointers */
int fb_covis_reserve_search_in_neighbors(fb_covis *g, int32_t n_mp, int32_t n_obs, int32_t new_edge_cap, int32_t kp_stride,
                                         int32_t n_targets, int32_t cand_cap, int32_t grid_cells);

/* ---- loop closing between the device calls: the consistency groups of DetectLoop (LoopClosing.cc:147-153, :155-228),
 * mvpLoopMapPoints (:355-375) and LoopConnections (:571-589).  Integer work on state the handle holds. ------------------- */
typedef struct fb_loop_groups_header {
  int32_t n_groups;             /* mvConsistentGroups.size() after the call (what fitted)                              */
  int32_t overflow;             /* != 0: more groups than cap_groups; what fitted is kept, nothing is written past it  */
} fb_loop_groups_header;
/* mvConsistentGroups lives on the handle, in a block of its own that the first of these calls allocates: up to cap_groups
 * groups (default max_keyframes; set ahead here), each a bitset over the slots of (max_keyframes + 31) / 32 words, bit
 * (slot & 31) of word (slot >> 5), and its consistency counter.  A call with another capacity than the block has makes a new
 * block: the groups are gone.  fb_covis_clear empties the groups.  fb_covis_erase_keyframe_dev does not touch them (the
 * reference's sets keep the pointer of a bad key frame), hence the precondition: a slot named in a live group is not handed
 * to another key frame while the groups live.                                                                            */
int fb_covis_reserve_loop_groups(fb_covis *g, int32_t cap_groups);
/* The consistency check that follows DetectLoopCandidates, on d_n_candidates[1] / d_candidates[] exactly as
 * fb_kfdb_query_dev wrote them (at most max_keyframes are read).  The group of candidate i is every slot with a non-zero
 * weight in its row -- entries below FB_COVIS_TH and non-members of the ordered vector included, as GetConnectedKeyFrames
 * returns them -- plus the candidate.  It is consistent with previous group g iff the two share a slot.  For each g only the
 * first consistent candidate pushes (its group, counter[g] + 1); a candidate consistent with no g pushes (its group, 0);
 * one consistent only with groups already taken pushes nothing.  The new list is candidate-major, then g ascending; the
 * same group may appear several times with different counters.  A candidate is enough when any consistent g has
 * counter[g] + 1 >= consistency_th (mnCovisibilityConsistencyTh, 3), taken or not: d_enough[max_keyframes] in candidate
 * order, d_n_enough[1]; entries past the count are left alone.  *d_n_candidates == 0 empties the groups (:147-153).  A
 * candidate outside [0, max_keyframes) is skipped and counted (fb_covis_error_count).  The early return on
 * mnId < mLastLoopKFid + 10 (:117-122) stays with the host, which does not call.  Enqueues only.  The two buffers swap on
 * the host side of the handle and the call's scratch lies in the same block, so consecutive calls (and fb_covis_loop_groups,
 * fb_covis_clear) must be on one stream or ordered by the caller with events; then they take effect in call order.       */
int fb_covis_detect_loop_dev(fb_covis *g, const int32_t *d_n_candidates, const int32_t *d_candidates, int32_t consistency_th,
                             int32_t *d_n_enough, int32_t *d_enough, fb_loop_groups_header *d_header, void *stream);
int fb_covis_detect_loop(fb_covis *g, const int32_t *n_candidates, const int32_t *candidates /* [max_keyframes] */,
                         int32_t consistency_th, int32_t *n_enough, int32_t *enough, fb_loop_groups_header *header); /* host pointers */
/* The groups as they stand: host pointers, waits for `stream`.  consistency[cap_groups] and bits[cap_groups][words] (either
 * may be NULL); *n entries are written.                                                                                  */
int fb_covis_loop_groups(fb_covis *g, int32_t *n, int32_t *consistency, uint32_t *bits, void *stream);

/* mvpLoopMapPoints (:355-375): GetVectorCovisibleKeyFrames() of matched_slot in the vector's order, then matched_slot;
 * within a key frame features ascending; a point is taken at its first occurrence if it is not NULL and not bad
 * (mnLoopPointForKF is the mark of one call).  A kf_mp entry >= n_mp is skipped and counted.  d_loop_mp[cap] holds point
 * indices as fb_search_and_fuse_args.d_loop_mp and fb_mp_list read them, d_n_loop[1] = min(count, cap), d_overflow[1] != 0
 * when the list did not fit (what fitted is written, nothing past cap).  The edge list of the map is not read.  Enqueues
 * only.                                                                                                                 */
int fb_covis_loop_map_points_dev(fb_covis *g, const fb_covis_map *map, int32_t matched_slot, int32_t cap, int32_t *d_n_loop,
                                 int32_t *d_loop_mp, int32_t *d_overflow, void *stream);
int fb_covis_loop_map_points(fb_covis *g, const fb_covis_map *map, int32_t matched_slot, int32_t cap, int32_t *n_loop,
                             int32_t *loop_mp, int32_t *overflow); /* host pointers */
/* its scratch ahead of time, behind the index the handle holds (as fb_covis_reserve_local_bird_map)                      */
int fb_covis_reserve_loop_map_points(fb_covis *g, int32_t n_mp);

typedef struct fb_loop_connections_header {
  int32_t total;                /* entries of LoopConnections over all rows                                            */
  int32_t overflow;             /* != 0: total > lc_cap; what fitted is written, nothing past lc_cap                   */
} fb_loop_connections_header;
typedef struct fb_loop_connections_args {
  int32_t set_cap;              /* rows of the batch (a launch parameter); 0 .. max_keyframes                          */
  const int32_t *d_n_set;       /* [1] mvpCurrentConnectedKFs.size(); min(*d_n_set, set_cap) members are processed     */
  const int32_t *d_set;         /* [set_cap] GetVectorCovisibleKeyFrames() of the current key frame, then the key frame */
  int32_t *d_n_counter;         /* [set_cap] } as fb_covis_update_connections_dev; rows past the list are left alone   */
  int32_t *d_front;             /* [set_cap] }                                                                         */
  int32_t lc_cap;
  int32_t *d_lc_off;            /* [set_cap + 1] CSR offsets (not clamped to lc_cap); rows past the list are empty     */
  int32_t *d_lc_slots;          /* [lc_cap] each row in ascending kf_order (a std::set<KeyFrame*>)                     */
  fb_loop_connections_header *d_header; /* [1]                                                                         */
} fb_loop_connections_args;
/* The pass that ends CorrectLoop (:571-589).  On the graph it is fb_covis_update_connections_dev over the list, in list
 * order; the caller follows with fb_covis_first_connection_dev and fb_covis_update_bird_connections_dev as documented
 * there.  Row j of LoopConnections = GetConnectedKeyFrames() of member j after its UpdateConnections (every entry of the
 * new row; with an empty counter the row stays and is what is read), minus vpPreviousNeighbors -- the members of its
 * ordered vector AT ITS TURN, after the AddConnections of the members before it, each of which rebuilds the vector of a
 * changed row from every entry -- minus the members of the list.  A slot outside [0, max_keyframes) gives an empty row and
 * is counted.  Enqueues only.                                                                                           */
int fb_covis_loop_connections_dev(fb_covis *g, const fb_covis_map *map, const fb_loop_connections_args *a, void *stream);
int fb_covis_loop_connections(fb_covis *g, const fb_covis_map *map, const fb_loop_connections_args *a); /* host pointers */
int fb_covis_reserve_loop_connections(fb_covis *g, int32_t n_mp, int32_t n_obs, int32_t set_cap);

/* ======================================================================== */
/* Frame geometry either side of the matchers (src/Frame.cc)                 */
/* ======================================================================== */
/* --- Frame::isInFrustum(pMP, viewingCosLimit) over a list of map points (Frame.cc:435-491; the loop
 *     around it is Tracking::SearchLocalPoints, Tracking.cc:1071-1091).  Outputs of a point that is
 *     not in view are left untouched, as the reference leaves the MapPoint's track members.        */
typedef struct fb_frustum_args {
  int32_t batch;
  int32_t mp_stride;
  const float *Tcw;             /* [batch][12] mRcw | mtcw                                           */
  const float *Ow;              /* [batch][3] mOw                                                    */
  const int32_t *n_mp;
  const uint8_t *mp_valid;      /* the caller's filter (not already matched, !isBad()); NULL = all   */
  const float *mp_xw;           /* [..][3]                                                           */
  const float *mp_normal;       /* [..][3] GetNormal()                                               */
  const float *mp_max_dist;     /* mfMaxDistance                                                     */
  const float *mp_min_dist;     /* mfMinDistance                                                     */
  fb_camera cam;
  float mbf;
  float viewing_cos_limit;      /* 0.5 at Tracking.cc:1084                                           */
  float log_scale_factor;
  int32_t n_levels;
  uint8_t *in_view;             /* mbTrackInView                                                     */
  float *proj;                  /* [..][2] mTrackProjX, mTrackProjY                                  */
  float *proj_xr;               /* mTrackProjXR; may be NULL                                         */
  int32_t *level;               /* mnTrackScaleLevel                                                 */
  float *view_cos;              /* mTrackViewCos                                                     */
} fb_frustum_args;
int fb_in_frustum_dev(const fb_frustum_args *args, void *stream);
int fb_in_frustum(const fb_frustum_args *args);

/* --- the geometric test of Tracking::FilterBirdOutlierInFront (Tracking.cc:1825-1914) over the bird matches of a
 *     frame pair: match i passes when |Tcw2 * (Twc1 * Xc1[query_i]) - Xc2[train_i]| < windowSize (:1868-1886) and its
 *     train slot holds no MapPointBird yet -- on entry (occupied2) or through an earlier passing match (:1861-1863).
 *     The MapPointBird bookkeeping (:1891-1903) stays with the caller, who walks `keep` in order.                  */
typedef struct fb_bird_filter_args {
  int32_t batch;
  int32_t match_stride, kp1_stride, kp2_stride;
  const int32_t *n_matches;       /* vDMatches12.size()                                              */
  const int32_t *query_idx;       /* [batch][match_stride] DMatch::queryIdx (frame 1)                */
  const int32_t *train_idx;       /* DMatch::trainIdx (frame 2)                                      */
  const float *cam_xyz1;          /* [batch][kp1_stride][3] MatchedFrame1->mvKeysBirdCamXYZ          */
  const float *cam_xyz2;          /* [batch][kp2_stride][3] MatchedFrame2->mvKeysBirdCamXYZ          */
  const float *Tcw1, *Tcw2;       /* [batch][12]                                                     */
  const uint8_t *occupied2;       /* [batch][kp2_stride] MatchedFrame2->mvpMapPointsBird[i] != NULL   */
  float window_size;
  uint8_t *keep;                  /* [batch][match_stride] 1 = pushed to newMatch                     */
  float *pt_world;                /* [batch][match_stride][3] ptwC (position of a new MapPointBird)   */
} fb_bird_filter_args;
int fb_bird_filter_matches_dev(const fb_bird_filter_args *args, void *stream);
int fb_bird_filter_matches(const fb_bird_filter_args *args);

/* --- Frame::UndistortKeyPoints (Frame.cc:636-669): cv::fisheye::undistortPoints(pts, K, D, R=I, P=K) on
 *     every key point; D[0]==0 copies.  K4 = fx,fy,cx,cy, D4 = k1..k4 (host).  d_kps_un may alias d_kps. */
int fb_undistort_keypoints_dev(const fb_keypoint *d_kps, const int32_t *d_n, int batch, int kp_stride,
                               const float *K4, const float *D4, fb_keypoint *d_kps_un, void *stream);
int fb_undistort_keypoints(const fb_keypoint *kps, int n, const float *K4, const float *D4,
                           fb_keypoint *kps_un); /* host pointers */
/* --- Frame::ComputeImageBounds (Frame.cc:741-795): bounds[4] = mnMinX, mnMaxX, mnMinY, mnMaxY.      */
int fb_image_bounds(int cols, int rows, const float *K4, const float *D4, float *bounds);

/* ======================================================================== */
/* Optimizer::PoseOptimization / PoseOptimizationWithBird / BirdOptimization */
/* (include/Optimizer.h:40-68, src/Optimizer.cc:246-835)                     */
/* ======================================================================== */
enum { FB_POSE_FRONT = 0, FB_POSE_FRONT_BIRD = 1, FB_POSE_BIRD = 2 };

typedef struct fb_pose_opt_args {
  int32_t batch;
  int32_t mode;          /* FB_POSE_*                                          */
  int32_t front_stride;  /* entries per problem in front_* arrays              */
  int32_t bird_stride;
  float fx, fy, cx, cy;
  float wF, wB;          /* Optimizer.h:52 defaults 1,1                        */
  /* front edges: one per mvpMapPoints[i] != NULL (Optimizer.cc:525-571)        */
  const int32_t *n_front;        /* [batch]                                    */
  const float *front_xw;         /* [..][3]                                    */
  const float *front_obs;        /* [..][2] kpUn.pt                            */
  const float *front_inv_sigma2; /* mvInvLevelSigma2[kpUn.octave]              */
  const uint8_t *front_valid;    /* slot i carries an edge (mvpMapPoints[i] != NULL); NULL = all */
  /* bird edges: one per mvpMapPointsBird[i] != NULL (Optimizer.cc:575-602)     */
  const int32_t *n_bird;
  const float *bird_xw;          /* [..][3]                                    */
  const float *bird_xc;          /* [..][3] mvKeysBirdCamXYZ                   */
  const float *bird_inv_sigma2;
  const uint8_t *bird_valid;     /* mvpMapPointsBird[i] != NULL; NULL = all       */
  uint8_t *bird_outlier;         /* in/out mvBirdOutlier (not reset by the reference) */
  /* pose in/out: pFrame->mTcw rows 0..2, row-major 3x4 float                   */
  float *Tcw;                    /* [batch][12]                                */
  uint8_t *front_outlier;        /* out mvbOutlier                             */
  int32_t *ninliers;             /* [batch] return value                       */
} fb_pose_opt_args;
int fb_pose_opt_batch_dev(const fb_pose_opt_args *args, void *stream);

/* inv_level_sigma2 of the first nlevels pyramid levels, by value (the edge builders' kernel argument) */
typedef struct fb_pose_gather_levels {
  float inv_sigma2[FB_MAX_LEVELS];
  int32_t nlevels;
} fb_pose_gather_levels;

/* Device-side form of the edge construction loops of PoseOptimizationWithBird
 * (Optimizer.cc:525-571 front, :575-602 bird): slot i of the frame becomes edge i.
 *   front: valid = match[i] >= 0, Xw = mp_xw[match[i]], obs = kps[i].pt,
 *          inv_sigma2 = inv_level_sigma2[kps[i].octave]
 *   bird : additionally Xc = cam_xyz[i]                                        */
int fb_pose_gather_front_dev(int batch, int kp_stride, int mp_stride, const int32_t *d_n,
                             const fb_keypoint *d_kps, const int32_t *d_match, const float *d_mp_xw,
                             const float *inv_level_sigma2 /* host, nlevels */, int nlevels,
                             float *d_front_xw, float *d_front_obs, float *d_front_inv_sigma2,
                             uint8_t *d_front_valid, void *stream);
int fb_pose_gather_bird_dev(int batch, int kp_stride, int mp_stride, const int32_t *d_n,
                            const fb_keypoint *d_kps, const float *d_cam_xyz, const int32_t *d_match,
                            const float *d_mpb_xw, const float *inv_level_sigma2, int nlevels,
                            float *d_bird_xw, float *d_bird_xc, float *d_bird_inv_sigma2,
                            uint8_t *d_bird_valid, void *stream);
int fb_pose_opt(const fb_pose_opt_args *args); /* host pointers */

/* The per-frame tail of the tracking step (Tracking.cc:292-339, 1312-1385), one launch per camera and one workgroup per
 * frame pair.  Each call computes exactly what the separate entry points it names compute, into the same arrays, byte for
 * byte; the cell lists, and for the bird camera mvKeysBirdCamXYZ, are still stored for the caller but go from stage to stage
 * in LDS.  m3.cur_cell_start / cur_cell_items (and m9.cur_cam_xyz) are declared const in the matcher structs and are
 * OUTPUTS here.
 *
 * fb_frame_tail_front_dev = fb_grid_build_batch_dev(m3.cur_kps, m3.n_cur, m3.grid -> m3.cur_cell_*)
 *                           -> fb_match_projection_frame_dev(&m3)
 *                           -> fb_pose_gather_front_dev(m3.match_cur_to_last, m3.last_xw -> front_*)
 *                           and n_front[b] = m3.n_cur[b], Tcw[b] = m3.cur_Tcw[b]  (SetPose(prediction), Tracking.cc:1314-1320) */
typedef struct fb_frame_tail_front_args {
  fb_proj_frame_args m3;
  fb_pose_gather_levels edge;    /* inv_level_sigma2 of the extractor, as fb_pose_gather_front_dev takes it */
  float *front_xw, *front_obs, *front_inv_sigma2; /* [batch][m3.cur_stride][3 | 2 | 1] edge i = key point slot i */
  uint8_t *front_valid;          /* [batch][m3.cur_stride], written over the whole stride                    */
  int32_t *n_front;              /* [batch]                                                                   */
  float *Tcw;                    /* [batch][12]                                                               */
} fb_frame_tail_front_args;
int fb_frame_tail_front_dev(const fb_frame_tail_front_args *args, void *stream);

/* fb_frame_tail_bird_dev  = fb_grid_build_batch_dev(m9.cur_kps, m9.n_cur, m9.grid -> m9.cur_cell_*)
 *                           -> fb_bird_keys_to_cam_dev(pixel2meter, m9.rear_axle_to_center, Tcb -> m9.cur_cam_xyz)
 *                           -> fb_match_bird_mappoints_dev(&m9) on m9.match_cur_to_ref = -1 over the whole stride
 *                              (mvpMapPointsBird of a new frame: the call sets it, no pre-fill)
 *                           -> fb_pose_gather_bird_dev(m9.match_cur_to_ref, m9.ref_xw -> bird_*)
 *                           and n_bird[b] = m9.n_cur[b], bird_outlier = 1 over the whole stride (Frame.cc:356) */
typedef struct fb_frame_tail_bird_args {
  fb_bird_mp_args m9;
  double pixel2meter;            /* Converter.cc:284-292                                                      */
  float Tcb[12];                 /* rows 0..2 of Frame::Tcb                                                   */
  fb_pose_gather_levels edge;
  float *bird_xw, *bird_xc, *bird_inv_sigma2;     /* [batch][m9.cur_stride][3 | 3 | 1]                        */
  uint8_t *bird_valid;           /* [batch][m9.cur_stride]                                                    */
  uint8_t *bird_outlier;         /* [batch][m9.cur_stride]                                                    */
  int32_t *n_bird;               /* [batch]                                                                   */
} fb_frame_tail_bird_args;
int fb_frame_tail_bird_dev(const fb_frame_tail_bird_args *args, void *stream);

/* ======================================================================== */
/* Device-resident Frame and the per-frame tracking chain                    */
/* (include/Frame.h, src/Frame.cc:262-379; src/Tracking.cc:1312-1441,690-746) */
/* ======================================================================== */
/* An fb_frame is the reference's Frame object for `batch` independent sequences, with every per-key-point member living
 * in HBM: mvKeys / mvKeysUn / mDescriptors / mGrid / mvpMapPoints / mvbOutlier, their bird counterparts (mvKeysBird,
 * mDescriptorsBird, mvKeysBirdCamXYZ, mGridBirdview, mvpMapPointsBird, mvBirdOutlier) and mTcw / mOw.  The entry points
 * below take frames where the reference's ORBmatcher / Optimizer methods take Frame& / Frame*, so that consecutive calls
 * (extract -> match -> optimise -> match -> optimise, and frame k -> frame k+1) hand their results over on the device.
 * mvpMapPoints[i] / mvpMapPointsBird[i] are kept as int32 indices into the caller's map tables (-1 = NULL).
 * The handle owns three device blocks: the members (what fb_frame_copy_dev copies), the BoW arrays (from the first
 * fb_frame_compute_bow_dev on) and the scratch its stages hand each other; fb_frame_view_dev points into the first.
 *
 * All *_dev entry points only enqueue on `stream`; the return values of the reference functions (match / inlier counts)
 * land in the frame's counter block, which fb_frame_counts reads back (one synchronisation per frame instead of one per
 * call).  The Tracking state machine stays with the host: it reads the counters and decides on retries (Tracking.cc:1345),
 * LOST handling and key-frame insertion.  One call at a time per frame handle.                                          */
typedef struct fb_frame fb_frame;

typedef struct fb_frame_params {
  int32_t batch;                    /* sequences side by side; 1 = the reference's single Frame                        */
  int32_t front_width, front_height, bird_width, bird_height;
  fb_orb_params orb;                /* ORBextractor.* of the settings file: capacity and level tables (Frame.cc:299-306)  */
  int32_t bird_nfeatures;           /* features of the bird extractor (the reference: cv::ORB::create(2000), Frame.cc:337;
                                       BASELINE configs[2]: 1000 bird edges); 0 = orb.nfeatures.  <= orb.nfeatures        */
  float K[4];                       /* Camera.fx, fy, cx, cy (Tracking.cc:61-75)                                        */
  float D[4];                       /* Camera.k1, k2, p1, p2, fed to the fisheye model as k1..k4 (Frame.cc:657);
                                       D[0] == 0: mvKeysUn = mvKeys (Frame.cc:640-644)                                  */
  float Tbc[12], Tcb[12];           /* Frame::Tbc / Tcb rows 0..2 (CalculateExtrinsics, Frame.cc:1015-1037)             */
  double pixel2meter, meter2pixel, rear_axle_to_center; /* Frame.cc:39-42                                               */
  int32_t map_cap;                  /* largest fb_map_points.stride a call may pass (per-point "seen" flags)            */
  int32_t local_mp_cap;             /* longest mvpLocalMapPoints list a call may pass (>= map stride for NULL lists)    */
  int32_t local_mpb_cap;            /* longest vlocalMPB list (>= bird map stride for NULL lists)                       */
} fb_frame_params;

/* The caller's MapPoint table on the device (MapPoint getters; the Map itself stays with the host, which refreshes the
 * entries LocalMapping changed).  An index into it is what a frame stores in mvpMapPoints.  [batch][stride] arrays.     */
typedef struct fb_map_points {
  int32_t stride;                   /* <= fb_frame_params.map_cap                                                       */
  const int32_t *n;                 /* [batch] entries in use                                                           */
  const uint8_t *bad;               /* isBad()                                                                          */
  const uint8_t *obs_pos;           /* Observations() > 0                                                               */
  const float *xw;                  /* [..][3] GetWorldPos()                                                            */
  const float *normal;              /* [..][3] GetNormal()                                                              */
  const float *max_dist, *min_dist; /* mfMaxDistance, mfMinDistance (the 1.2 / 0.8 factors are applied by the kernels)  */
  const uint8_t *desc;              /* [..][32] GetDescriptor()                                                         */
} fb_map_points;

/* MapPointBird table.  FilterBirdOutlierInFront creates points (Tracking.cc:1896-1901): they are appended at n[b].     */
typedef struct fb_map_points_bird {
  int32_t stride;
  int32_t *n;                       /* [batch] entries in use (in/out)                                                  */
  float *xw;                        /* [..][3] GetWorldPos()                                                            */
  uint8_t *desc;                    /* [..][32] mDescriptor                                                             */
} fb_map_points_bird;

/* slots of a frame's counter block */
enum {
  FB_CNT_BIRD_KF_MATCHES = 0, /* mnBirdKFMatches = BirdMapPointMatch(...)            Tracking.cc:2006                   */
  FB_CNT_PROJ_MATCHES,        /* nmatches = SearchByProjection(cur, last)            Tracking.cc:1339                   */
  FB_CNT_POSE1_INLIERS,       /* PoseOptimizationWithBird                            Tracking.cc:1353                   */
  FB_CNT_MATCHES,             /* nmatches after the outlier discard                  Tracking.cc:1358-1376              */
  FB_CNT_MATCHES_MAP,         /* nmatchesMap                                         Tracking.cc:1373                   */
  FB_CNT_BIRDVIEW_MATCHES,    /* nmatchesBird = BirdviewMatch(...)                   Tracking.cc:2728                   */
  FB_CNT_BIRD_INLIERS,        /* inlier of FilterBirdOutlierInFront                  Tracking.cc:1888                   */
  FB_CNT_BIRD_NEW,            /* mnBirdLastFMatches = buildNew                       Tracking.cc:1913                   */
  FB_CNT_TO_MATCH,            /* nToMatch of SearchLocalPoints                       Tracking.cc:1973-1982              */
  FB_CNT_LOCAL_MATCHES,       /* SearchByProjection(cur, mvpLocalMapPoints, th)      Tracking.cc:1995                   */
  FB_CNT_POSE2_INLIERS,       /* PoseOptimizationWithBird                            Tracking.cc:1400                   */
  FB_CNT_MATCHES_INLIERS,     /* mnMatchesInliers                                    Tracking.cc:1411-1424              */
  FB_CNT_BOW_MATCHES,         /* nmatches = SearchByBoW(mpReferenceKF, cur, ...)     Tracking.cc:1207                   */
  FB_CNT_BIRD_POINTS,         /* numPt = GetBirdMapPointsNum()                       Tracking.cc:1196                   */
  FB_CNT_PROJ_RETRIED,        /* 1 = SearchByProjection ran again with 2 * th        Tracking.cc:1342-1349              */
  FB_CNT_BIRD_POINTS_FINAL,   /* GetBirdMapPointsNum() after the last GetPerFrameMatchedBirdPoints of the frame
                                 (numPt of BirdNeedKF, Tracking.cc:2067)                                                */
  FB_CNT_COUNT = 16
};

int fb_frame_create(const fb_frame_params *params, fb_frame **out);
void fb_frame_destroy(fb_frame *f);

/* Frame::Frame(imGray, BirdGray, ..., birdviewmask, ..., birdviewContourICP, ...) (Frame.cc:262-379) on images in HBM:
 * ExtractORB (front) -> UndistortKeyPoints -> bird extraction (ORBextractor, the E9 substitution) with the detect mask
 * -> GuidenceKeyBirdPts on d_contour -> mvKeysBirdCamXYZ -> mvpMapPoints = NULL, mvbOutlier = false, mvpMapPointsBird =
 * NULL, mvBirdOutlier = TRUE (:355-356) -> AssignFeaturesToGrid.  Image b starts b * image_stride bytes after the base;
 * d_contour / d_mask have the bird image's geometry (rows of bird_stride bytes) and may be NULL (no filter / no mask).
 * The bird chain runs on a stream the handle owns, forked from and joined back into `stream` inside the call.           */
int fb_frame_extract_dev(fb_frame *f, fb_orb *front_extractor, fb_orb *bird_extractor, const uint8_t *d_front,
                         int front_stride, size_t front_image_stride, const uint8_t *d_bird, int bird_stride,
                         size_t bird_image_stride, const uint8_t *d_contour, const uint8_t *d_mask, void *stream);
/* The same from HOST images (the reference's call): the images are copied through page-locked staging buffers the handle
 * owns, asynchronously on `stream`; the call returns when the copies out of the caller's buffers are done, not when the
 * kernels are (fb_frame_counts / fb_frame_download synchronise).  Images are tightly packed batch after batch.           */
int fb_frame_extract(fb_frame *f, fb_orb *front_extractor, fb_orb *bird_extractor, const uint8_t *front, int front_stride,
                     const uint8_t *bird, int bird_stride, const uint8_t *contour, const uint8_t *mask, void *stream);

/* cv::cornerSubPix on the bird key points inside fb_frame_extract[_dev] (Frame.cc:345-352): with half_win in 1..8 every
 * later extraction runs fb_corner_subpix_dev(half_win, half_win, max_iter, eps) on the handle's bird stream after the
 * guidance filter (straight after the extraction when there is no contour) and before mvKeysBirdCamXYZ and the bird grid,
 * which are therefore built from the refined positions.  half_win = 0 switches it off again; off is the state of a new
 * handle.  Descriptors stay those of the unrefined positions unless fb_frame_set_bird_redescribe is on as well.  A
 * refined point outside the image stays a key point and falls in no grid cell (PosInGridBirdview).                       */
int fb_frame_set_bird_subpix(fb_frame *f, int32_t half_win, int32_t max_iter, double eps);

/* extractorBird->compute(BirdGray, mvKeysBird, mDescriptorsBird) at the refined positions (Frame.cc:352-355): with on != 0
 * AND fb_frame_set_bird_subpix on, every later extraction runs fb_orb_describe_dev(bird_extractor, FB_DESCRIBE_KEEP_ANGLE)
 * on the frame's bird key points and descriptors (the arrays the guidance filter has compacted) on the handle's bird
 * stream, straight after fb_corner_subpix_dev.  A key point whose refined position lies outside the 19-px border of its
 * level keeps the descriptor of its unrefined position, stays a key point at its index (no compaction, see
 * fb_orb_describe_args) and has the status FB_DESCRIBE_BORDER.  With cornerSubPix off the switch does nothing: the
 * descriptors are already those of the positions.  Off is the state of a new handle; turning it on allocates the
 * [batch][fb_orb_capacity] status bytes the handle owns.                                                                 */
int fb_frame_set_bird_redescribe(fb_frame *f, int32_t on);
/* The detector of the bird image (Frame.cc:337-340).  FB_BIRD_DETECT_ORBEXTRACTOR (the state of a new handle): the bird
 * extractor's own fb_orb_extract_batch_dev, as always.  FB_BIRD_DETECT_CVORB: every later extraction runs, on
 * the handle's bird stream and with no added synchronisation, the reference's chain Frame.cc:337-355 on the bird extractor:
 *   fb_orb_detect_masks_dev(fast_threshold) with the detect mask of each image applied at every level (cv::ORB::detect);
 *   fb_bird_guidance_dev with mask = NULL (the mask is already applied) when there is a contour image;
 *   fb_corner_subpix_dev when fb_frame_set_bird_subpix is on;
 *   fb_orb_describe_dev(FB_DESCRIBE_KEEP_ANGLE), always: this detector does not describe.  It runs whatever
 *   fb_frame_set_bird_redescribe says, and fb_frame_download_bird_describe_status returns its status bytes (a point that
 *   cornerSubPix moved outside the 19-px border of its level is FB_DESCRIBE_BORDER and its descriptor row is unspecified).
 * nfeatures, nlevels and scale_factor are the bird extractor's; at most fb_orb_capacity entries per image are kept (ties
 * beyond it are cut off in output order).  A detect mask without a contour image is refused as before.  Turning CVORB on
 * allocates the status bytes the handle owns.  fast_threshold: 1..255 (cv::ORB's default is 20).                         */
enum { FB_BIRD_DETECT_ORBEXTRACTOR = 0, FB_BIRD_DETECT_CVORB = 1 };
int fb_frame_set_bird_detector(fb_frame *f, int32_t mode, int32_t fast_threshold);

/* The status bytes (FB_DESCRIBE_*) of the last extraction that re-described, host_status [batch][fb_orb_capacity]; only
 * the entries below n_bird are meaningful.  FB_ERR_ARG when the frame's last extraction did not re-describe.
 * Synchronises `stream`.                                                                                                 */
int fb_frame_download_bird_describe_status(fb_frame *f, uint8_t *host_status, void *stream);

/* Frame::SetPose(Tcw) + UpdatePoseMatrices (Frame.cc:421-433): d_Tcw [batch][12] device.                                */
int fb_frame_set_pose_dev(fb_frame *f, const float *d_Tcw, void *stream);
/* mCurrentFrame.SetPose(detlaT * mLastFrame.mTcw) (Tracking.cc:1314-1320): d_delta [batch][12] = rows 0..2 of detlaT.   */
int fb_frame_predict_pose_dev(fb_frame *cur, const fb_frame *last, const float *d_delta, void *stream);
/* fill(mvpMapPoints, NULL) (Tracking.cc:1330,1344)                                                                       */
int fb_frame_clear_map_points_dev(fb_frame *f, void *stream);
/* A frame that enters the chain without having been tracked (the first one after initialisation): sets mvpMapPoints /
 * mvpMapPointsBird from host-built index arrays [batch][fb_orb_capacity] (device), mvbOutlier = false.                  */
int fb_frame_set_map_points_dev(fb_frame *f, const int32_t *d_map_point, const int32_t *d_map_point_bird, void *stream);

/* BirdMapPointMatch(CurF, vlocalMPB, windowSize, filterSize) (ORBmatcher.cc:1763-1902, Tracking.cc:1999-2012; M9).
 * d_local [batch][params.local_mpb_cap] lists vlocalMPB as indices into `mpb`, d_n_local [batch] their counts; NULL
 * lists = the whole table in index order.  Tracking.cc:2004: the call is skipped (count 0) unless the list has > 10
 * entries.                                                                                                              */
int fb_frame_bird_mappoint_match_dev(fb_frame *cur, const fb_map_points_bird *mpb, const int32_t *d_local,
                                     const int32_t *d_n_local, int window_size, float filter_size,
                                     const fb_matcher_params *matcher, void *stream);
/* SearchByProjection(CurrentFrame, LastFrame, th, bMono = true) (ORBmatcher.cc:1329-1471; M3)                           */
int fb_frame_search_by_projection_dev(fb_frame *cur, const fb_frame *last, const fb_map_points *map, float th,
                                      const fb_matcher_params *matcher, void *stream);
/* PoseOptimization / PoseOptimizationWithBird / BirdOptimization(pFrame) (Optimizer.cc:246-835), mode FB_POSE_*.
 * which = 0 writes FB_CNT_POSE1_INLIERS, 1 writes FB_CNT_POSE2_INLIERS.                                                 */
int fb_frame_pose_optimization_dev(fb_frame *f, const fb_map_points *map, const fb_map_points_bird *mpb, int mode,
                                   float wB, float wF, int which, void *stream);
/* "Discard outliers" of TrackWithMotionModel (Tracking.cc:1358-1376).  A dropped point is marked as seen in this frame
 * (pMP->mnLastFrameSeen = mCurrentFrame.mnId, :1370): the mark is a byte per map point ON THE FRAME HANDLE (`map` stays
 * read-only), it is what fb_frame_search_local_points_dev skips, fb_frame_copy_dev copies it, a further discard in the
 * same frame adds to it, and only fb_frame_extract[_dev] (a new Frame, a new mnId) clears it.                           */
int fb_frame_discard_outliers_dev(fb_frame *f, const fb_map_points *map, void *stream);
/* GetPerFrameMatchedBirdPoints (Tracking.cc:2724-2733): BirdviewMatch(cur, ref keys / descriptors, ..., 0, window)
 * (M8) followed by the whole of FilterBirdOutlierInFront(ref, cur, matches, filter_size) (:1825-1914), bookkeeping
 * included: cur.mvBirdOutlier[train] = false, cur.mvpMapPointsBird[train] = ref's point or a NEW MapPointBird (appended
 * to `mpb` with position ptwC and cur's descriptor) that ref.mvpMapPointsBird[query] receives as well.                  */
int fb_frame_match_bird_points_dev(fb_frame *cur, fb_frame *ref, fb_map_points_bird *mpb, int window_size,
                                   float filter_size, const fb_matcher_params *matcher, void *stream);
/* SearchLocalPoints (Tracking.cc:1947-1997): points the frame already holds are marked seen -- like the points the
 * discard loops of this frame dropped (the marks fb_frame_discard_outliers_dev and the fused stages leave on the handle;
 * :1974: neither projected, nor counted in FB_CNT_TO_MATCH, nor matched again) --, isInFrustum(pMP, 0.5) on the
 * others of mvpLocalMapPoints (d_local: indices into `map`, [batch][params.local_mp_cap]; NULL = the whole table), then
 * SearchByProjection(cur, mvpLocalMapPoints, th) (ORBmatcher.cc:46-130; M2) if anything is to be matched.               */
int fb_frame_search_local_points_dev(fb_frame *f, const fb_map_points *map, const int32_t *d_local,
                                     const int32_t *d_n_local, float th, const fb_matcher_params *matcher, void *stream);
/* End of Tracking::Track for a tracked frame (Tracking.cc:1411-1424 mnMatchesInliers; :690-701 clean VO matches;
 * :721-725 mvpMapPoints[i] = NULL for outliers) -- after it the frame is what mLastFrame = Frame(mCurrentFrame) copies. */
int fb_frame_finish_dev(fb_frame *f, const fb_map_points *map, void *stream);
/* (both end-of-Track entry points follow `if (bOK)` of Tracking.cc:681 per sequence: the clean-up runs where
 * FB_CNT_MATCHES_INLIERS >= 30, Tracking.cc:1438; a sequence below keeps its members, as a LOST frame does)
 * Tracking.cc:721-725 on its own, after a key-frame decision (fb_track_args.defer_outlier_drop). */
int fb_frame_drop_outliers_dev(fb_frame *f, void *stream);

/* The OK-state path of Tracking::Track in one call: TrackWithMotionModel (Tracking.cc:1312-1385) + TrackLocalMap
 * (:1387-1441) + the end-of-Track clean-up, i.e. predict_pose, M9, M3 (th = 15), PoseOptimizationWithBird, discard,
 * M8 + filter (window 10, 0.05 m), SearchLocalPoints (th = 1, nnratio 0.8), PoseOptimizationWithBird, finish --
 * per sequence as the reference does: the 2 * th retry of :1342-1349 runs inside the matcher launch, and a sequence that
 * still has fewer than 20 matches "returns false" (:1351): its matches stay committed, pose and flags are left alone.   */
typedef struct fb_track_args {
  fb_map_points map;
  fb_map_points_bird mpb;
  const float *d_delta;             /* [batch][12] detlaT                                                               */
  const int32_t *d_local_mp, *d_n_local_mp;   /* mvpLocalMapPoints (NULL = whole table)                                 */
  const int32_t *d_local_mpb, *d_n_local_mpb; /* vlocalMPB (NULL = whole table)                                         */
  float wB, wF;                     /* Optimizer.h:52 defaults 1, 1                                                     */
  /* fb_frame_track_local_map_dev: 1 = per sequence `if (bOK) bOK = TrackLocalMap()` (Tracking.cc:642): a sequence whose first
   * stage returned false (FB_CNT_MATCHES_MAP < 10; the counter is still 0 after an early return) is left alone -- no bird
   * points created, no matching, pose and flags untouched, counters of the stage 0.  0 = every sequence of the handle runs
   * (the host decided for all of them).  fb_frame_track_dev always gates.                                               */
  int32_t gate_local_map;
  /* 1 = leave the final "mvpMapPoints[i] = NULL for outliers" (Tracking.cc:721-725) to fb_frame_drop_outliers_dev: the
   * reference creates its key frame in between (:716-718) and lets the outliers pass to it.                              */
  int32_t defer_outlier_drop;
  /* TrackLocalMap's success threshold on mnMatchesInliers: 0 = 30 (Tracking.cc:1438); a host that relocalised less than
   * mMaxFrames frames ago passes 50 (:1435-1436).                                                                        */
  int32_t min_inliers;
} fb_track_args;
int fb_frame_track_dev(fb_frame *cur, fb_frame *last, const fb_track_args *args, void *stream);
/* The two halves of fb_frame_track_dev on their own, for a host that reads the counters in between (Tracking.cc:529-540:
 * bOK = TrackWithMotionModel(); if (!bOK) bOK = TrackReferenceKeyFrame(); ... if (bOK) bOK = TrackLocalMap()):
 *   fb_frame_track_motion_model_dev  Tracking::TrackWithMotionModel (Tracking.cc:1312-1385); bOK = FB_CNT_MATCHES_MAP >= 10
 *   fb_frame_track_local_map_dev     Tracking::TrackLocalMap (:1387-1441, ref = tmpRefFrame) + the end of Track (:690-725)  */
int fb_frame_track_motion_model_dev(fb_frame *cur, fb_frame *last, const fb_track_args *args, void *stream);
int fb_frame_track_local_map_dev(fb_frame *cur, fb_frame *ref, const fb_track_args *args, void *stream);
/* Tracking::UpdateLocalMap (Tracking.cc:1394, :2085-2229) for the frames of the handle: fb_covis_local_map_dev with batch,
 * kp_stride, d_n and d_map_point taken from the frame and cap_mp = local_mp_cap (those fields of `a` are ignored).  Its
 * d_local_mp / d_n_local_mp are exactly what fb_track_args.d_local_mp / d_n_local_mp read.  The frame's map point indices
 * index the one map of `map`.                                                                                           */
int fb_frame_update_local_map_dev(fb_frame *cur, fb_covis *g, const fb_covis_map *map, const fb_local_map_args *a, void *stream);
/* fb_frame_track_dev with the list derived from the frame between its two halves, no synchronisation:
 * TrackWithMotionModel -> UpdateLocalMap -> the rest of TrackLocalMap, the last two gated per sequence on
 * FB_CNT_MATCHES_MAP >= 10 (a's own gate fields are ignored).  args->d_local_mp / d_n_local_mp must be a->d_local_mp /
 * a->d_n_local_mp (FB_ERR_ARG otherwise).                                                                              */
int fb_frame_track_graph_dev(fb_frame *cur, fb_frame *last, const fb_track_args *args, fb_covis *g, const fb_covis_map *map,
                             const fb_local_map_args *a, void *stream);

/* Tracking::TrackUsingBird (Tracking.cc:2014-2061: the frame of a LOST tracker that could not re-initialise, bHaveBird):
 * SetPose(detlaT * src pose) with src = mpReferenceKF's handle (IsbirdWithRefKF == 1) or tmpRefFrame, GetLocalMapForBird,
 * GetPerFrameMatchedBirdPoints against `ref` first for the sequences with numPt <= 10 (FB_CNT_BIRD_POINTS),
 * Optimizer::BirdOptimization(&frame, 1.0) (bird edges only; inliers -> FB_CNT_POSE1_INLIERS), GetPerFrameMatchedBirdPoints. */
int fb_frame_track_using_bird_dev(fb_frame *cur, fb_frame *src, fb_frame *ref, const fb_track_args *args, void *stream);

/* Frame(const Frame &) (Frame.cc:49-82: tmpRefFrame = new Frame(mCurrentFrame), Tracking.cc:746) and the member copies of
 * KeyFrame::KeyFrame(Frame &F, ...) (KeyFrame.cc:32-91): every member array of src into dst (same parameters), device to
 * device on the stream, including the BoW when src has it and the frame's seen marks (fb_frame_discard_outliers_dev).
 * A handle owns its member arrays as one block and the BoW arrays as a second: the copy is one transfer of each.
 * FB_ERR_ARG unless both handles were created with the same batch, orb parameters (capacity) and map_cap: the arrays
 * are copied whole.                                                                                                     */
int fb_frame_copy_dev(fb_frame *dst, const fb_frame *src, void *stream);

/* Frame::ComputeBoW (Frame.cc:628-635; KeyFrame::ComputeBoW, KeyFrame.cc:93-102) on the handle: transform(mDescriptors,
 * mBowVec, mFeatVec, 4) into buffers the handle owns; a second call on the same frame is a no-op (if (mBowVec.empty())),
 * fb_frame_extract* empties them again.  voc = device arrays.  fb_frame_bow_view_dev hands out the device pointers
 * (fb_bow_transform_args layout, f_stride = kp_stride).                                                                  */
int fb_frame_compute_bow_dev(fb_frame *f, const fb_vocabulary *voc, void *stream);
int fb_frame_bow_view_dev(fb_frame *f, fb_bow_transform_args *view);
/* ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches) (ORBmatcher.cc:160-289) with the key frame given as the frame handle
 * it was made from (KeyFrame.cc:32-91 copies mvKeysUn, mDescriptors, mvpMapPoints): count -> FB_CNT_BOW_MATCHES, then
 * mCurrentFrame.mvpMapPoints = vpMapPointMatches (Tracking.cc:1215) for the sequences with count >= min_matches (the
 * others keep their mvpMapPoints, Tracking.cc:1212-1213).  Both frames need their BoW (FB_ERR_ARG otherwise).             */
int fb_frame_search_by_bow_dev(fb_frame *cur, const fb_frame *kf, const fb_map_points *map, const fb_matcher_params *matcher,
                               int min_matches, void *stream);
/* Tracking::TrackReferenceKeyFrame (Tracking.cc:1180-1244, bLooseCouple = true, bHaveBird): SetPose(detlaT * kf pose) with
 * args->d_delta = detlaT of :1185, GetLocalMapForBird, GetPerFrameMatchedBirdPoints against `ref` (tmpRefFrame) for the
 * sequences holding fewer than 10 bird points (count -> FB_CNT_BIRD_POINTS; FB_CNT_BIRDVIEW_MATCHES reads 0 where the
 * step was skipped), ComputeBoW, SearchByBoW(0.7), and for the sequences with >= 15 matches: mvpMapPoints = matches,
 * PoseOptimizationWithBird (FB_CNT_POSE1_INLIERS), the outlier discard (FB_CNT_MATCHES, FB_CNT_MATCHES_MAP).  The
 * reference's return value per sequence = FB_CNT_BOW_MATCHES >= 15 && FB_CNT_MATCHES_MAP >= 10; a sequence below 15 keeps
 * its predicted pose, members and the two discard counters, like the early return.                                       */
int fb_frame_track_reference_dev(fb_frame *cur, fb_frame *kf, fb_frame *ref, const fb_vocabulary *voc, const fb_track_args *args,
                                 void *stream);

/* Pointers to a frame's arrays: device pointers from fb_frame_view_dev (valid for the handle's lifetime, for harnesses
 * that keep working on the device), or host buffers the caller hands to fb_frame_download (NULL members are skipped).
 * kp_stride = fb_orb_capacity(params.orb).                                                                             */
typedef struct fb_frame_view {
  int32_t batch, kp_stride;
  int32_t *n;                       /* [batch] N                                                                        */
  fb_keypoint *kps, *kps_un;        /* mvKeys, mvKeysUn                                                                 */
  uint8_t *desc;                    /* mDescriptors                                                                     */
  int32_t *map_point;               /* mvpMapPoints as table index, -1 = NULL                                           */
  uint8_t *outlier;                 /* mvbOutlier                                                                       */
  int32_t *n_bird;                  /* [batch] Nbird                                                                    */
  fb_keypoint *kps_bird;            /* mvKeysBird                                                                       */
  uint8_t *desc_bird;               /* mDescriptorsBird                                                                 */
  float *bird_cam_xyz;              /* mvKeysBirdCamXYZ                                                                 */
  int32_t *map_point_bird;          /* mvpMapPointsBird                                                                 */
  uint8_t *bird_outlier;            /* mvBirdOutlier                                                                    */
  float *Tcw;                       /* [batch][12]                                                                      */
  int32_t *counts;                  /* [FB_CNT_COUNT][batch] (slot-major: every kernel writes one contiguous row)      */
} fb_frame_view;
int fb_frame_view_dev(fb_frame *f, fb_frame_view *out);
/* mGridBirdview as the CSR fb_grid_build_batch_dev writes (32 x 32 cells) into host buffers [batch][1025] and
 * [batch][kp_stride]; synchronises `stream`.                                                                              */
int fb_frame_download_bird_grid(fb_frame *f, int32_t *host_cell_start, int32_t *host_cell_items, void *stream);
int fb_frame_download(fb_frame *f, const fb_frame_view *host, void *stream); /* synchronises `stream`                  */
int fb_frame_counts(fb_frame *f, int32_t *host_counts /* [FB_CNT_COUNT][batch] */, float *host_Tcw /* [batch][12] or NULL */,
                    void *stream);                                              /* synchronises `stream`                 */

/* ======================================================================== */
/* Optimizer::LocalBundleAdjustment / LocalBundleAdjustmentWithOdom          */
/* (src/Optimizer.cc:838-1165, 2137-2670)                                    */
/* ======================================================================== */
typedef struct fb_local_ba_args {
  int32_t with_odom;   /* 0: LocalBundleAdjustment (SE3Expmap edges), 1: ...WithOdom (Quat edges + bird + odom) */
  float fx, fy, cx, cy;
  float wF, wB, wP;
  int32_t n_kf;               /* local + fixed keyframes, graph insertion order */
  float *kf_Tcw;              /* in/out [n_kf][12]                              */
  const uint8_t *kf_fixed;    /* [n_kf]                                         */
  int32_t n_mp;
  float *mp_xw;               /* in/out [n_mp][3]                               */
  int32_t n_mpb;
  float *mpb_xw;              /* in/out [n_mpb][3]                              */
  /* front observations, grouped by map point in insertion order */
  int32_t n_obs;
  const int32_t *obs_kf;      /* index into kf                                  */
  const int32_t *obs_mp;      /* index into mp                                  */
  const float *obs_uv;        /* [n_obs][2]                                     */
  const float *obs_inv_sigma2;
  /* bird observations */
  int32_t n_bobs;
  const int32_t *bobs_kf;
  const int32_t *bobs_mpb;
  const float *bobs_xc;       /* [n_bobs][3]                                    */
  const float *bobs_inv_sigma2;
  /* odometry edges (Optimizer.cc:2419-2495) */
  int32_t n_odom;
  const int32_t *odom_kf_i;
  const int32_t *odom_kf_j;
  const float *odom_Tij;      /* [n_odom][12]                                   */
  const double *odom_info;    /* information scale per edge (1e4*wP, 2e3, 1e3*wP) */
  const volatile uint8_t *stop_flag; /* host-visible pbStopFlag, may be NULL    */
  uint8_t *obs_outlier;       /* out [n_obs]                                    */
  uint8_t *bobs_outlier;      /* out [n_bobs]                                   */
} fb_local_ba_args;
int fb_local_ba(const fb_local_ba_args *args); /* host pointers */
/* The same with the graph resident in HBM (the LocalMapping-side chain hands its results over on the device: triangulation
 * matches -> new points -> fuse -> local BA, LocalMapping.cc:62-99): kf_Tcw, mp_xw, mpb_xw, every obs_* / bobs_* array and the
 * two outlier arrays are DEVICE pointers; kf_fixed, the odometry edges (odom_*: at most 3 n_kf of them) and stop_flag stay
 * HOST pointers (the window comes from the host or from fb_covis_local_window_dev, Optimizer.cc:2139-2227; the host builds
 * the odometry chain, :2419-2495).  The edge records, the CSR by landmark / by
 * key frame and the duplicate check are built by kernels on `stream`, ordered behind the producers of the arrays; results are
 * written back on `stream`.  The call returns when the optimisation has finished (the schedule's length is data dependent:
 * the host watches the device-resident Levenberg-Marquardt loop), like the reference's blocking call.
 * Capacity: <= 23 free key frames, <= 32768 observations per key frame (larger graphs: fb_local_ba).                       */
int fb_local_ba_dev(const fb_local_ba_args *args, void *stream);

/* Optimizer::BundleAdjustmentWithOdom / GlobalBundleAdjustemntWithOdom (Optimizer.cc:1778-2135) on the same graph
 * description: with_odom = 1 (Quat edges), n_odom = 0 (the pose-graph block is commented out in the reference,
 * :2004-2037), kf_fixed[k] = (mnId == 0).  ONE optimize(nIterations) (:2048-2050), Huber delta sqrt(5.99) on every edge
 * iff bRobust (:1836,1891-1895,1980-1984), no chi2 classification: obs_outlier / bobs_outlier are not written.
 * Capacity (local and global BA alike): up to 23 free key frames the Schur-reduced pose system is LDS resident
 * (MFMA Schur kernel + one-workgroup LDL^T); beyond that it lives in HBM (block scatter + blocked multi-kernel LDL^T),
 * up to 682 free key frames.                                                                                        */
int fb_global_ba(const fb_local_ba_args *args, int n_iterations, int robust);

/* One local BA over `world` GPUs (one process per GPU), SURVEY 8(e): rank r owns the landmarks l with
 * l % world == r and all their edges, odometry edges live on rank 0, keyframes are replicated.  Every rank
 * passes the SAME complete problem and receives the complete result.  The library calls `allreduce` (the
 * only callback of this ABI) to combine `n` doubles in host memory in place over the ranks: op 0 = sum,
 * 1 = max.  Two calls per LM trial: the Schur-reduced pose system, then [Hpp, bp, chi2, scale].       */
typedef int (*fb_allreduce_fn)(void *ctx, double *buf, int32_t n, int32_t op);
int fb_local_ba_sharded(const fb_local_ba_args *args, int rank, int world, fb_allreduce_fn allreduce, void *ctx);

/* The same with RCCL inside the library: the two exchanges of an LM trial are ncclAllReduce calls on device buffers,
 * enqueued on the BA's stream between its kernels (no host staging, no read-back: the Levenberg-Marquardt state machine
 * runs on the device and takes identical decisions on every rank from the reduced values; pbStopFlag and a rank's
 * argument errors travel inside the reduced buffers so that every branch is collective).  `comm` is an ncclComm_t over
 * the `world` ranks.  RCCL is resolved at run time (dlopen of librccl.so.1: torch's when the host is Python), so the
 * library has no link-time dependency on it; fb_rccl_* wrap ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy of that
 * same RCCL for hosts that do not own a communicator yet (rank 0 makes the id, the host broadcasts its 128 bytes).  */
typedef struct fb_rccl_unique_id { char internal[128]; } fb_rccl_unique_id;
int fb_rccl_get_unique_id(fb_rccl_unique_id *id);
int fb_rccl_comm_init(const fb_rccl_unique_id *id, int rank, int world, void **comm);
int fb_rccl_comm_destroy(void *comm);
/* ncclCommCount / ncclCommUserRank of a communicator: what RCCL itself says about the ranks it connects (bench.py prints it
 * as local_ba.rccl_ranks_seen, so that a multi-GPU run shows that the collective really spans the ranks). */
int fb_rccl_comm_info(void *comm, int *count, int *rank);
int fb_local_ba_sharded_rccl(const fb_local_ba_args *args, int rank, int world, void *comm);

#ifdef __cplusplus
}
#endif
#endif /* FISHBIRD_H_ */
