/*
 * vtf.h — C ABI of libvtf_hip.so, the MI355X-native hot path of video-to-faces.
 *
 * The reference has no C ABI: its plugin surface is Python.  These entry
 * points are what that Python surface binds to (video-to-faces_amd/videotofaces/_native.py,
 * ctypes); each names the reference interface it replaces.  Conventions:
 *   - every call returns int status: 0 = ok, negative = error (message: vtf_last_error());
 *   - no exceptions cross the ABI; the caller owns every buffer it passes;
 *   - "d_" pointers are device (HBM) pointers, others are host pointers;
 *   - a handle is bound to one GPU and one HIP stream (vtf_*_set_stream) and is not
 *     thread-safe (the reference calls its models from one Python thread).
 */
#ifndef VTF_H
#define VTF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VTF_OK 0
#define VTF_E_ARG (-1)        /* bad argument (shape, null pointer, ...)           */
#define VTF_E_HIP (-2)        /* HIP runtime error                                 */
#define VTF_E_CAPACITY (-3)   /* output buffer too small; *out_total says how big  */
#define VTF_E_DEGENERATE (-4) /* reference crop loop would skip a box -> IndexError */
#define VTF_E_LIMIT (-5)      /* an internal size limit was exceeded               */

const char* vtf_last_error(void);
/* Free the library's per-stream scratch (box ops, dedupe, conv tail workspaces) of a HIP
 * stream the caller is about to destroy; waits for the stream.  Long-lived processes that
 * create streams per request call this so device memory stays bounded. */
int vtf_release_stream(void* hip_stream);
int vtf_version(void);

typedef struct vtf_mtcnn_s* vtf_mtcnn_t;
typedef struct vtf_facenet_s* vtf_facenet_t;
typedef struct vtf_vit_s* vtf_vit_t;
typedef struct vtf_yolo_s* vtf_yolo_t;
typedef struct vtf_group_s* vtf_group_t;
typedef struct vtf_rcnn_s* vtf_rcnn_t;

/* Box post-processing parameters (video_to_faces det_min_score, det_min_size, det_min_border,
 * det_scale, det_square; main.py:50-51), see vtf_boxes_to_crops. */
typedef struct vtf_box_params {
    float min_score;   /* compared in fp32 (numpy float32 vs Python float, NEP 50) */
    double min_size;   /* width or height below -> rejected */
    double min_border; /* 0 = no border check */
    double scale[4];   /* sx1, sx2, sy1, sy2 */
    int32_t square;
    int32_t adjust;    /* 1: adjust_boxes after filter_boxes (the pipeline); 0: filter_boxes only */
} vtf_box_params;

/* ---------------------------------------------------------------- MTCNN detector
 * Replaces RealMTCNN / MTCNN.forward (src/videotofaces/detectors/mtcnn.py:167-252,
 * 312-326), called by detection.py:131 `detout = model(frames)`.
 * params: fp32, the reference state_dict order minus num_batches_tracked
 *         (videotofaces/specs.py mtcnn_spec, 495,850 floats). */
int vtf_mtcnn_create(const float* params, int64_t n_params, int device, vtf_mtcnn_t* out);
int vtf_mtcnn_destroy(vtf_mtcnn_t h);
int vtf_mtcnn_set_stream(vtf_mtcnn_t h, void* hip_stream);

/* frames: uint8 BGR, frame b pixel (y,x) channel c at frames[b*frame_stride + y*row_stride
 * + x*3 + c] (a borrowed, possibly non-contiguous view, detection.py:114-116).
 * frames_on_device: 1 if `frames` is a device pointer.
 * Output (host): boxes [total,5] (x1,y1,x2,y2,score), landmarks [total,5,2] ((x,y) per point, as
 * mtcnn.py:239 stacks them; may be NULL), counts[B]; per image in reference order.  If total > cap nothing is
 * written, *out_total is set and VTF_E_CAPACITY returned. */
int vtf_mtcnn_detect(vtf_mtcnn_t h, const uint8_t* frames, int frames_on_device, int B, int H, int W,
                     int64_t frame_stride, int64_t row_stride, double min_face_size,
                     float* out_boxes, float* out_landmarks, int32_t* out_counts, int64_t cap,
                     int64_t* out_total);

/* detect + box post-processing with nothing on the host but the counts: the detector's rows
 * stay in HBM and go through vtf_boxes_to_crops (detection.py:131-145).  frames as above;
 * d_crops / out_frame_counts / cap / out_n as in vtf_boxes_to_crops. */
int vtf_mtcnn_detect_crops(vtf_mtcnn_t h, const uint8_t* frames, int frames_on_device, int B, int H, int W,
                           int64_t frame_stride, int64_t row_stride, double min_face_size,
                           const vtf_box_params* params, int32_t frame_offset, int32_t* d_crops,
                           int32_t* out_frame_counts, int64_t cap, int64_t* out_n);

/* Per-stage counters of the last detect call: [0] levels, [1] stage-1 candidates (all
 * levels), [2] after per-level NMS, [3] after cross-level NMS (= stage-2 proposals),
 * [4] stage-2 passing, [5] after stage-2 NMS (= stage-3 refinements), [6] stage-3 passing,
 * [7] final faces. */
int vtf_mtcnn_stats(vtf_mtcnn_t h, int64_t* out8);

/* Parity introspection (tests): enable = 1 / 0 turns recording of the stage-1 candidate set on /
 * off for later detect calls (-1 leaves it), then the last call's stage-1 keys -- (level << 32 |
 * (b * ph + y) * pw + x) of every cell with p >= 0.6, ascending = the reference's per-level
 * nonzero() order (mtcnn.py:183-186) -- are copied to out (up to cap) and their count to *out_n. */
int vtf_mtcnn_stage1_keys(vtf_mtcnn_t h, int enable, uint64_t* out, int64_t cap, int64_t* out_n);

/* Parity introspection (tests): the last detect call's PNet plan (pnet_exact_tiles) -- per pyramid
 * level 1 if the exact-levels kernel is planned to take it (the launch still falls back to the
 * general kernel on VTF_PNET_X=0), else 0 -- copied to out (up to cap), the level count to *out_n. */
int vtf_mtcnn_pnet_plan(vtf_mtcnn_t h, int32_t* out, int64_t cap, int64_t* out_n);

/* Kernel timing of the dominant kernel (fused pyramid+PNet) with HIP events recorded on the
 * handle's stream around each launch.  enable=1 resets and starts accumulating; the call
 * returns the totals so far: elapsed ms, launches, algorithmic FLOPs (2*MAC of conv1-3 and
 * the heads over every pyramid level) and frames. */
int vtf_mtcnn_profile(vtf_mtcnn_t h, int enable, double* out_ms, int64_t* out_launches, double* out_flops,
                      int64_t* out_frames);

/* Parity entry points (device pointers, handle stream).
 * Fused MTCNN._resample + PNet for one pyramid level (mtcnn.py:150-151, 27-38):
 * d_prob [B,ph,pw], d_reg [B,4,ph,pw] with ph = ceil((lh-2)/2)-4. */
int vtf_mtcnn_pnet_level(vtf_mtcnn_t h, const uint8_t* d_frames, int B, int H, int W, int64_t frame_stride,
                         int64_t row_stride, int lh, int lw, float* d_prob, float* d_reg);
/* MTCNN._resample of the preprocessed frames (mtcnn.py:133-139,150-151): d_out [B,3,lh,lw]. */
int vtf_mtcnn_resample(vtf_mtcnn_t h, const uint8_t* d_frames, int B, int H, int W, int64_t frame_stride,
                       int64_t row_stride, int lh, int lw, float* d_out);
/* RNet / ONet on given fp32 NCHW inputs (mtcnn.py:58-76, 101-121). */
int vtf_mtcnn_rnet(vtf_mtcnn_t h, const float* d_in, int64_t n, float* d_reg, float* d_prob);
int vtf_mtcnn_onet(vtf_mtcnn_t h, const float* d_in, int64_t n, float* d_reg, float* d_lm, float* d_prob);

/* ---------------------------------------------------------------- box post-processing
 * process_frames_batch steps 2-5 (src/videotofaces/detection.py:133-145) on device:
 * filter_boxes (detection.py:174-217, with check_box 165-171), adjust_boxes (220-262) and the
 * (frame, face) flatten of get_crops (161-162).  Parameters as video_to_faces passes them
 * (main.py:50-51): det_min_score, det_min_size, det_min_border, det_scale (sx1, sx2, sy1, sy2),
 * det_square. */

/* d_rows: device fp32 [n,5] (x1,y1,x2,y2,score) grouped by frame, counts: host int32 [B] rows per
 * frame (negative = frame absent from the detector output: no crops).  Writes device int32
 * d_crops [m,5] (frame_offset + frame, x1, y1, x2, y2) in row order, d_src [m] (source row, may be
 * NULL), host out_frame_counts [B] (may be NULL) and *out_n = m.  VTF_E_CAPACITY when the rows
 * exceed cap (then *out_n = rows, nothing written). */
int vtf_boxes_to_crops(const float* d_rows, const int32_t* counts, int B, int H, int W, const vtf_box_params* params,
                       int32_t frame_offset, int32_t* d_crops, int32_t* d_src, int32_t* out_frame_counts,
                       int64_t cap, int64_t* out_n, void* hip_stream);

/* ---------------------------------------------------------------- box ops
 * torchvision.ops.batched_nms as called at mtcnn.py:196,205,219 and
 * detectors/operations/post.py:8: d_boxes [n,4] fp32, d_scores [n], d_idxs [n] int64.
 * Writes keep indices (int64, score-descending) to d_keep and their count to *out_nkeep. */
int vtf_batched_nms(const float* d_boxes, const float* d_scores, const int64_t* d_idxs, int64_t n,
                    double iou_threshold, int64_t* d_keep, int64_t* out_nkeep, void* hip_stream);

/* MTCNN._nms_vectorized(boxes, scores, classes, thr, 'Min') with chain suppression
 * (mtcnn.py:273-309, called at 242): rows sorted by descending score (ties in index order:
 * the reference's argsort is unstable there), a row is dropped when ANY earlier row of the same
 * class overlaps it with intersection-over-minimum (+1 pixel widths) > thr (fp32).
 * d_boxes [n,4] fp32, d_scores [n], d_classes [n] int32 -> d_keep int64 (kept rows in that
 * order), *out_nkeep. */
int vtf_iom_nms(const float* d_boxes, const float* d_scores, const int32_t* d_classes, int64_t n, float thr,
                int64_t* d_keep, int64_t* out_nkeep, void* hip_stream);

/* ---------------------------------------------------------------- FaceNet encoder
 * Replaces FaceNet / InceptionResnetV1 (src/videotofaces/encoders/facenet.py:123-183),
 * called by grouping.py:37 `xk = model(images)`.
 * precision: 0 = fp32 (parity mode), 1 = bf16 activations/weights with fp32 accumulation. */
int vtf_facenet_create(const float* params, int64_t n_params, int device, int precision, vtf_facenet_t* out);
int vtf_facenet_destroy(vtf_facenet_t h);
int vtf_facenet_set_stream(vtf_facenet_t h, void* hip_stream);
/* Encoder on blob input: d_x [N,3,160,160] fp32 NCHW RGB (cv2.dnn.blobFromImages output,
 * facenet.py:179) -> d_emb [N,512] fp32, L2-normalised. */
int vtf_facenet_forward(vtf_facenet_t h, const float* d_x, int64_t N, float* d_emb);
/* Crop + resize + normalise faces straight from device frames (blobFromImages(1/128,
 * 160x160, 127.5, swapRB) on each crop, INTER_LINEAR uint8), then encode.
 * d_frames: F device frames as in vtf_mtcnn_detect; crops int32 [N,5] (frame index, x1, y1,
 * x2, y2) in frame pixels (detection.py:161-162 get_crops slices), a host array (validated:
 * 0 <= frame < F, non-empty slice inside the frame, else VTF_E_ARG) or, with crops_on_device,
 * a device array such as vtf_*_detect_crops writes (read by the kernel; an invalid rectangle
 * encodes a zero image instead of reading outside the frames). */
int vtf_facenet_encode_crops(vtf_facenet_t h, const uint8_t* d_frames, int F, int H, int W, int64_t frame_stride,
                             int64_t row_stride, const int32_t* crops, int crops_on_device, int64_t N,
                             float* d_emb);
/* Blob of uint8 BGR crops (cv2.dnn.blobFromImages, INTER_LINEAR, swapRB): d_out [N,3,S,S].
 * out = (resized_u8 - mean) * scale.  d_crops: device int32 [N,5] into F frames. */
int vtf_blob_from_crops(const uint8_t* d_frames, int F, int H, int W, int64_t frame_stride, int64_t row_stride,
                        const int32_t* d_crops, int64_t N, int S, float mean, float scale, float* d_out,
                        void* hip_stream);

/* ---------------------------------------------------------------- ViT encoder
 * Replaces ViT / AnimeVIT (src/videotofaces/encoders/vit.py:80-146), called by grouping.py:37.
 * dim 768 / depth 12 (B16) or 1024 / 24 (L16); params in the reference state_dict order
 * (specs.py vit_spec).  fp32 or guarded split-fp16 (vtf_vit_set_precision). */
int vtf_vit_create(const float* params, int64_t n_params, int dim, int depth, int device, vtf_vit_t* out);
int vtf_vit_destroy(vtf_vit_t h);
int vtf_vit_set_stream(vtf_vit_t h, void* hip_stream);
/* GEMM operand mode: 0 = fp32 MFMA (default); 2 = fp32 operands split into two fp16 parts on the
 * fp16 matrix cores (fp32-grade products), guarded: an operand >= 2^14 re-runs the forward in fp32. */
int vtf_vit_set_precision(vtf_vit_t h, int mode);
/* d_x [N,3,128,128] fp32 blob (blobFromImages(1/127.5, 128x128, 127.5, swapRB)) -> d_emb [N,dim]
 * (LayerNorm of the CLS token, not L2-normalised). */
int vtf_vit_forward(vtf_vit_t h, const float* d_x, int64_t N, float* d_emb);
/* crops as in vtf_facenet_encode_crops, resized to 128x128 (vit.py:141). */
int vtf_vit_encode_crops(vtf_vit_t h, const uint8_t* d_frames, int F, int H, int W, int64_t frame_stride,
                         int64_t row_stride, const int32_t* crops, int crops_on_device, int64_t N, float* d_emb);

/* fp32-grade GEMM on the fp16 matrix cores (the split-fp16 ViT Linear layers, vit.py:29-37):
 * out[M,N] = a[M,K] b[N,K]^T (+ bias[N]); device fp32 row-major operands, split on device into
 * x0 + x1 * 2^-11 fp16 pairs (|x| < 2^14 required: VTF_E_ARG otherwise).  K % 32 == 0, N % 8 == 0.
 * Stream-ordered; returns after the stream is synchronised. */
int vtf_gemm_split(const float* d_a, const float* d_b, int64_t M, int N, int K, const float* d_bias, float* d_out,
                   void* hip_stream);

/* One convolution of the implicit-GEMM conv engine (csrc/conv.hip, conv_dma.hip) on dense fp32
 * device buffers: the direct entry the kernel tests use.  The call packs the operands into the
 * layout of `mode`, launches what production dispatch picks (path 0) or the named kernel
 * configuration, and decodes the outputs to fp32.  Output buffers are read, taken through the
 * kernel's layout and written back, never cleared: pre-fill them.
 *   d_in  [N][H][W][in_cstride or Cin], d_w [Cout][KH][KW][Cin]
 *   d_out [N][OH][OW][out_cstride] ([N][2 OH][2 OW][out_cstride] with up2)
 *   ovf   host int32: 1 when a split-fp16 producer met |x| >= 2^14 (f16x / sp modes)
 *   plan  host int32[8]: kernel id (0: nothing launched), BM, BN, dp_tiles, tail_split, split,
 *         parts, cg of what ran (the ids are `path`'s values)
 * Stream-ordered; returns after the stream is synchronised. */
enum { VTF_CONV_FP32 = 0, VTF_CONV_F16X = 1, VTF_CONV_SP = 2, VTF_CONV_BF16 = 3, VTF_CONV_S3 = 4 };
typedef struct vtf_conv2d_opts {
    const float* bias;  /* device [Cout] or null */
    const float* alpha; /* device [Cout] or null: v = fmaf(v, alpha, beta) */
    const float* beta;
    const float* prelu; /* device [Cout] or null */
    const float* res;   /* device dense fp32 [N][OH][OW][Cout] ([N][OH/2][OW/2][Cout] with res_up2) or null */
    float* out2;        /* device dense fp32 [N][OH][OW][out2_cstride] (n_split), pre-filled */
    float* pool_out;    /* device dense fp32 [N][POH][POW][Cout] (pool_k > 0), pre-filled */
    float scale, slope; /* scale 1 = off */
    int32_t relu, leaky, gelu, res_post, res_up2, up2;
    int32_t in_cstride, out_cstride, out_coff;
    int32_t n_split, out2_cstride, out2_coff;
    int32_t out_f32, split_fp32, out_sp;
    int32_t mode;       /* VTF_CONV_* */
    int32_t path;       /* 0 auto; 1-6 k_conv 128x32x32, 128x64x32 (fp32 / f16x), 64x32x64, 64x64x64,
                         * 32x32x64, 32x64x64 (bf16); 10-13 k_conv_dma bf16 256x32, 256x64, 128x128,
                         * 64x64 3-stage; 20-21 k_conv_dma split pairs 128x64, 128x128; 30 k_conv_span;
                         * 31 k_conv_span_pool (plan only); 40-41 k_conv_dma3 128x64, 64x128 */
    int32_t pool_k, pool_s; /* pool_k > 0: MaxPool2d(k, s, ceil_mode) after the conv (sp mode) */
    int32_t pool_fused;     /* 1: launch_conv_span_pool (d_out may be null); 0: the conv, then launch_maxpool_ks_sp */
} vtf_conv2d_opts;
int vtf_conv2d(const float* d_in, const float* d_w, int N, int H, int W, int Cin, int Cout, int KH, int KW, int sh, int sw,
               int ph, int pw, const vtf_conv2d_opts* opts, float* d_out, int32_t* ovf, int32_t* plan, void* hip_stream);

/* ---------------------------------------------------------------- grouping
 * remove_dupes_overall 'enc' branch (dupes.py:51-68 with sklearn cosine_distances):
 * for each row i, min and argmin over j < i of clip(1 - cos(X_i, X_j), 0, 2); row 0 gets
 * 10000 / 0 (the reference's masked diagonal).  d_X [N,D] fp32 -> d_min [N], d_arg [N]. */
int vtf_cosine_dedupe(const float* d_X, int64_t N, int64_t D, float* d_min, int64_t* d_arg, void* hip_stream);
/* The same for rows [row_begin, row_end) only (a rank's shard of the lower triangle, SURVEY.md
 * §8e): row_begin a multiple of 128, row_end a multiple of 128 or N; d_min / d_arg hold
 * row_end - row_begin entries.  Rows at or after row_end are not read. */
int vtf_cosine_dedupe_rows(const float* d_X, int64_t N, int64_t D, int64_t row_begin, int64_t row_end, float* d_min,
                           int64_t* d_arg, void* hip_stream);
/* classify (grouping.py:50-55): min / first argmin over c of sklearn cosine_distances(X, R)[i, c]
 * in sklearn's own bits (normalize; X_n @ R_n.T as numpy's OpenBLAS sgemm / sgemv / sdot orders;
 * clip(1 - G, 0, 2)).  d_X [N,D], d_R [C,D] fp32 -> d_min [N] fp32, d_arg [N] int64. */
int vtf_cosine_classify(const float* d_X, int64_t N, const float* d_R, int64_t C, int64_t D, float* d_min,
                        int64_t* d_arg, void* hip_stream);
/* the full matrix dist = cosine_distances(X, R) of classify (grouping.py:51) in the same bits:
 * d_dist [N,C] fp32 (the per-class distances of log_classification.csv, grouping.py:58-64). */
int vtf_cosine_distances_xr(const float* d_X, int64_t N, const float* d_R, int64_t C, int64_t D, float* d_dist,
                            void* hip_stream);

/* ---------------------------------------------------------------- hash dedupe
 * dupes.ahash (dupes.py:11-15) of N face crops of device frames (frames as in
 * vtf_mtcnn_detect (F frames), crops host int32 [N,5] = frame, x1, y1, x2, y2 as get_crops slices them
 * (validated as in vtf_facenet_encode_crops),
 * detection.py:161-162): out_hashes host uint64 [N], bit k = 8x8 thumbnail pixel k (row-major)
 * > mean.  cvtColor(BGR2GRAY) + resize INTER_LINEAR restated from OpenCV's fixed point. */
int vtf_ahash_crops(const uint8_t* d_frames, int F, int H, int W, int64_t frame_stride, int64_t row_stride,
                    const int32_t* crops, int64_t N, uint64_t* out_hashes, void* hip_stream);
/* remove_dupes_overall('hash') distances (dupes.py:55-64): for row i, min and first argmin over
 * j < i of popcount(h_i ^ h_j); row 0 -> 10000, 0.  d_hashes uint64 [N] -> d_min int32 [N],
 * d_arg int64 [N]. */
int vtf_hamming_dedupe(const uint64_t* d_hashes, int64_t N, int32_t* d_min, int64_t* d_arg, void* hip_stream);

/* ---------------------------------------------------------------- face files
 * cv2.imwrite(path, crop) of detection.py:155-158 on device: baseline JFIF, 4:2:0, libjpeg's
 * bytes.  frames / crops (host int32 [N,5], validated) as in vtf_ahash_crops.  quality 1..100.
 * d_out: device bytes, file i at [out_offsets[i], out_offsets[i+1]); out_offsets host int64
 * [N+1].  If the files need more than cap bytes nothing is written, *out_total says how many,
 * VTF_E_CAPACITY.  Returns after the stream is synchronised (the offsets are host values).
 * VTF_E_ARG: a null pointer, quality outside 1..100, an empty rectangle or one outside the frame,
 * a bad frame index.  N = 0 is fine (out_offsets[0] = 0).  Scratch: the stream's arena
 * (vtf_release_stream). */
int vtf_jpeg_encode_crops(const uint8_t* d_frames, int F, int H, int W, int64_t frame_stride, int64_t row_stride,
                          const int32_t* crops, int64_t N, int quality, uint8_t* d_out, int64_t cap,
                          int64_t* out_offsets, int64_t* out_total, void* hip_stream);
/* vtf_jpeg_encode_crops (the same files, offsets and errors) that also leaves, for every crop, the
 * BGR pixels libjpeg decodes from the crop's file: reconstructed on the device from the quantised
 * coefficients the encoder holds, so no file is entropy-decoded for them.  d_pixels: device bytes,
 * crop i as tight [h][w][3] rows at byte offset sum over j < i of h_j * w_j * 3 (any alignment);
 * pixels_cap below that sum over all crops: VTF_E_ARG.  out_status host int32 [N]: 0, or 2 for a
 * crop whose reconstruction left the int16 range (never for coefficients of 8-bit pixels); its
 * pixels are then unspecified.  With VTF_E_CAPACITY d_pixels is not written either.  The same
 * number of host syncs as vtf_jpeg_encode_crops. */
int vtf_jpeg_encode_crops_decoded(const uint8_t* d_frames, int F, int H, int W, int64_t frame_stride,
                                  int64_t row_stride, const int32_t* crops, int64_t N, int quality, uint8_t* d_out,
                                  int64_t cap, int64_t* out_offsets, int64_t* out_total, uint8_t* d_pixels,
                                  int64_t pixels_cap, int32_t* out_status, void* hip_stream);

/* cv2.imread(path) of grouping.py:29-40 on device: baseline 4:2:0 face files -> libjpeg's pixels.
 * A file is decoded on the device if it is SOF0, 8-bit, three components sampled 2x2 / 1x1 / 1x1,
 * one interleaved scan (Ss 0, Se 63, Ah = Al = 0), 8-bit DQT, any DHT tables, no restart interval,
 * no Adobe APP14 segment, EXIF orientation absent or 1 (what cv2.imwrite, Pillow's defaults and
 * vtf_jpeg_encode_crops write).  Everything else is classified on the host and reaches no kernel.
 *
 * vtf_jpeg_probe: host only, no GPU: parses one file's headers.  Never reads outside
 * [data, data + len).  info[8]:
 *   [0] h, [1] w (0 when no frame header was read)
 *   [2] kind: 0 = decodable on the device, 1 = a JPEG with whole headers but unsupported,
 *             2 = not a JPEG, or the headers end before the scan starts
 *   [3] scan_begin, [4] scan_end: the entropy-coded bytes [begin, end) relative to data; the scan
 *       ends at the first 0xFF that is not followed by 0x00, or at len (kind 0 and 1 only)
 *   [5] why (kind 1): bits 1 not SOF0, 2 sample / DQT precision, 4 not three YCbCr components, 8 sampling,
 *       16 restart interval, 32 Adobe segment, 64 EXIF orientation, 128 scan parameters or more than
 *       EOI after the scan, 256 missing or malformed table, 512 size
 *   [6] number of components, [7] 0 */
int vtf_jpeg_probe(const uint8_t* data, int64_t len, int32_t* info);
/* N files, host bytes back to back (file i at [offsets[i], offsets[i+1])), decoded into N slots of
 * a device uint8 BGR buffer [N][Hmax][Wmax][3] at the given strides (bytes).  One H2D copy of the
 * bytes.  A file writes only rows < h and columns < w of its slot.  out_sizes host int32 [N,2] =
 * (h, w); out_status host int32 [N]: 0 ok, 1 unsupported, 2 corrupt (or not a JPEG), 3 larger than
 * Hmax x Wmax (slot untouched for 1 and 3, its Hmax x Wmax pixels zero-filled for 2).  A per-file
 * problem is reported in out_status, not as the return code.  VTF_E_ARG: null pointers, N < 0,
 * decreasing offsets, strides too small.  N = 0 is fine.  Returns after the stream is
 * synchronised.  Scratch: the stream's arena (vtf_release_stream). */
int vtf_jpeg_decode(const uint8_t* data, const int64_t* offsets, int64_t N, uint8_t* d_bgr, int Hmax, int Wmax,
                    int64_t frame_stride, int64_t row_stride, int32_t* out_sizes, int32_t* out_status,
                    void* hip_stream);
/* vtf_jpeg_decode with a stage 1 made for long scans (video frames): every file's scan is cut
 * into segments of seg_bytes (after removing the stuffed zero bytes) and decoded by as many lanes of
 * one workgroup, which find their decoder states by speculation and re-synchronisation
 * (csrc/jpeg_entropy_split.hpp); stage 2 is the same.  The contract is vtf_jpeg_decode's: the same
 * classification on the host, sizes, statuses, slot rules, zero-fill of a corrupt file's slot and
 * argument errors; N = 0 is fine; returns after the stream is synchronised.  seg_bytes: 0 = the
 * library's default (128), otherwise a multiple of 4 in [4, 4096], else VTF_E_ARG.  The pixels do
 * not depend on seg_bytes. */
int vtf_jpeg_decode_split(const uint8_t* data, const int64_t* offsets, int64_t N, uint8_t* d_bgr, int Hmax, int Wmax,
                          int64_t frame_stride, int64_t row_stride, int32_t* out_sizes, int32_t* out_status,
                          int seg_bytes, void* hip_stream);
/* Faces that are in HBM already into the slots of such a buffer: faces host array [N] of device
 * pointers to tight [h][w][3] pixels (vtf_jpeg_encode_crops_decoded's), sizes host int32 [N,2] =
 * (h, w); face i is copied to rows < h and columns < w of slot i of d_atlas [N][Hmax][Wmax][3] at
 * the given strides (bytes), nothing else is written.  A null entry of faces leaves its slot alone
 * (the caller fills it; its size is not looked at).  One launch.  VTF_E_ARG: null arguments, N < 0,
 * h > Hmax, w > Wmax, strides too small (vtf_jpeg_decode's rule).  N = 0 is fine.  Returns after
 * the stream is synchronised.  Scratch: the stream's arena (vtf_release_stream). */
int vtf_faces_to_atlas(const uint8_t* const* faces, const int32_t* sizes, int64_t N, uint8_t* d_atlas, int Hmax,
                       int Wmax, int64_t frame_stride, int64_t row_stride, void* hip_stream);
/* cv2.resize(crop, (w, h)) INTER_LINEAR of resize_keep_ratio (utils/image.py:4-14, detection.py:147-148)
 * for N crops of device frames into the slots of such a buffer.  frames / crops (host int32 [N,5],
 * validated) as in vtf_ahash_crops; sizes host int32 [N,2] = the destination (h, w) of every crop.
 * Crop i is resampled to sizes[i] and written to rows < h and columns < w of slot i of d_atlas
 * [N][Hmax][Wmax][3] at the given strides (bytes); nothing else of a slot is written.  The pixels
 * are OpenCV's uint8 fixed point (11-bit coefficients) as utils.resize_linear restates it, bit for
 * bit; a destination equal to the source size copies the crop; an exact 2x downscale is
 * INTER_LINEAR too (no INTER_AREA substitution).  The atlas with the rectangles (i, 0, 0, w, h) is
 * a valid frames / crops input of vtf_ahash_crops and vtf_jpeg_encode_crops.  One launch.
 * VTF_E_ARG: null pointers, N < 0, a destination side < 1 or above Hmax / Wmax, an empty source
 * crop or one outside the frames, a bad frame index, atlas strides too small (vtf_jpeg_decode's
 * rule); nothing is written then.  N = 0 is fine and launches nothing.  Returns after the stream
 * is synchronised.  Scratch: the stream's arena (vtf_release_stream). */
int vtf_resize_crops(const uint8_t* d_frames, int F, int H, int W, int64_t frame_stride, int64_t row_stride,
                     const int32_t* crops, const int32_t* sizes, int64_t N, uint8_t* d_atlas, int Hmax, int Wmax,
                     int64_t atlas_frame_stride, int64_t atlas_row_stride, void* hip_stream);
/* Stage timing of vtf_jpeg_decode and vtf_jpeg_decode_split on the calling thread: enable != 0
 * makes later calls bracket their kernels with HIP events; out_ms (may be null) receives the last
 * timed call's (entropy decode, IDCT + upsampling + colour) milliseconds. */
int vtf_jpeg_decode_profile(int enable, float* out_ms);

/* ---------------------------------------------------------------- video frames
 * The decode side of process_video (src/videotofaces/detection.py:68-111, which hands the
 * detector cv2.VideoCapture / decord BGR frames [B,H,W,3]): planar YUV frames in HBM (as a
 * YUV4MPEG2 stream stores them: Y [H][W], then U and V planes of the chroma size) -> uint8 BGR.
 * d_yuv: n frames at in_frame_stride bytes; chroma 420 / 422 / 444 / 400 (mono, U = V = 128);
 * full_range 0 = BT.601 limited range (OpenCV's COLOR_YUV2BGR_I420 integer transform), 1 = full
 * range; chroma sampled nearest.  d_bgr: [n][H][W][3] at the given frame / row strides (bytes).
 * Asynchronous on hip_stream. */
int vtf_yuv_to_bgr(const uint8_t* d_yuv, int64_t n, int H, int W, int chroma, int full_range, int64_t in_frame_stride,
                   uint8_t* d_bgr, int64_t out_frame_stride, int64_t out_row_stride, void* hip_stream);

/* ---------------------------------------------------------------- YOLOv3 detector
 * Replaces RealYOLO / YOLOv3.forward (src/videotofaces/detectors/yolo.py:131-191), called by
 * detection.py:131 `detout = model(frames)`.
 * params: fp32, reference state_dict order minus num_batches_tracked (specs.py yolo_spec,
 *         61,576,342 floats).  precision 0 = fp32 (parity), 1 = bf16 operands/activations. */
int vtf_yolo_create(const float* params, int64_t n_params, int device, int precision, vtf_yolo_t* out);
int vtf_yolo_destroy(vtf_yolo_t h);
int vtf_yolo_set_stream(vtf_yolo_t h, void* hip_stream);
/* frames as in vtf_mtcnn_detect.  Output (host): boxes [total,4] (x1,y1,x2,y2 in frame
 * pixels, unclamped), scores [total], counts[B] (<= 100 each); per image in the reference's
 * order (score desc).  Classes are all 0 (num_classes=1).  VTF_E_CAPACITY as in mtcnn. */
int vtf_yolo_detect(vtf_yolo_t h, const uint8_t* frames, int frames_on_device, int B, int H, int W,
                    int64_t frame_stride, int64_t row_stride, float* out_boxes, float* out_scores,
                    int32_t* out_counts, int64_t cap, int64_t* out_total);
/* detect + box post-processing on device, as vtf_mtcnn_detect_crops. */
int vtf_yolo_detect_crops(vtf_yolo_t h, const uint8_t* frames, int frames_on_device, int B, int H, int W,
                          int64_t frame_stride, int64_t row_stride, const vtf_box_params* params,
                          int32_t frame_offset, int32_t* d_crops, int32_t* out_frame_counts, int64_t cap,
                          int64_t* out_n);
/* resize_cv2 keep-ratio size (prep.py:71-73) and the x32 padded net input: {h, w, Hp, Wp}. */
int vtf_yolo_input_size(int H, int W, int* out4);
/* Parity entries.  letterbox: preprocess (prep.py:12-92) -> d_out NHWC fp32 [B,Hp,Wp,8]
 * (channels 3..7 zero).  net: d_x NCHW fp32 [B,3,Hp,Wp] -> pred maps NHWC fp32
 * [B,Hp/32,Wp/32,18], [B,Hp/16,Wp/16,18], [B,Hp/8,Wp/8,18] (yolo.py:143-145).
 * postprocess: the maps of frames of size HxW -> detect's outputs (yolo.py:146-147). */
int vtf_yolo_letterbox(vtf_yolo_t h, const uint8_t* d_frames, int B, int H, int W, int64_t frame_stride,
                       int64_t row_stride, float* d_out);
int vtf_yolo_net(vtf_yolo_t h, const float* d_x, int B, int Hp, int Wp, float* d_map0, float* d_map1,
                 float* d_map2);
int vtf_yolo_postprocess(vtf_yolo_t h, const float* d_map0, const float* d_map1, const float* d_map2, int B,
                         int H, int W, float* out_boxes, float* out_scores, int32_t* out_counts, int64_t cap,
                         int64_t* out_total);
/* Conv-stack timing (HIP events around the 75 conv launches of each detect/net call):
 * accumulated ms, launches, algorithmic FLOPs and frames since the last call; enable != 0
 * turns timing on for the following calls. */
int vtf_yolo_profile(vtf_yolo_t h, int enable, double* out_ms, int64_t* out_launches, double* out_flops,
                     int64_t* out_frames);

/* ---------------------------------------------------------------- Faster R-CNN detector
 * Replaces AnimeFRCNN / FasterRCNN.forward (src/videotofaces/detectors/rcnn.py:127-177),
 * called by detection.py:131 `detout = model(frames)` for style='anime'.
 * params: fp32, reference state_dict order minus num_batches_tracked (specs.py rcnn_spec,
 *         41,401,301 floats).  precision 0 = fp32 (parity), 1 = bf16 operands/activations. */
int vtf_rcnn_create(const float* params, int64_t n_params, int device, int precision, vtf_rcnn_t* out);
int vtf_rcnn_destroy(vtf_rcnn_t h);
int vtf_rcnn_set_stream(vtf_rcnn_t h, void* hip_stream);
/* frames as in vtf_mtcnn_detect.  Output (host): boxes [total,4] (x1,y1,x2,y2 in frame pixels),
 * scores [total], counts[B] (<= 100 each), per image in the reference's order (score desc).
 * counts[b] = -1 for images after the last one holding an RPN proposal: the reference returns
 * only max(imidx)+1 lists (rcnn.py:111).  Classes are all 0.  VTF_E_CAPACITY as in mtcnn. */
int vtf_rcnn_detect(vtf_rcnn_t h, const uint8_t* frames, int frames_on_device, int B, int H, int W,
                    int64_t frame_stride, int64_t row_stride, float* out_boxes, float* out_scores,
                    int32_t* out_counts, int64_t cap, int64_t* out_total);
/* detect + box post-processing on device, as vtf_mtcnn_detect_crops (frames past the last
 * proposal image produce no crops, as the reference's shorter detout list does). */
int vtf_rcnn_detect_crops(vtf_rcnn_t h, const uint8_t* frames, int frames_on_device, int B, int H, int W,
                          int64_t frame_stride, int64_t row_stride, const vtf_box_params* params,
                          int32_t frame_offset, int32_t* d_crops, int32_t* out_frame_counts, int64_t cap,
                          int64_t* out_n);
/* resize_cv2 keep-ratio size for resize=(800, 1333) (prep.py:71-74) and the x32 padded net
 * input: {h, w, Hp, Wp}. */
int vtf_rcnn_input_size(int H, int W, int* out4);
/* Parity entries.  preprocess (prep.py:12-92, imagenet mean/std) -> d_out NHWC fp32
 * [B,Hp,Wp,8] (channels 3..7 zero).  rpn_heads: body + FPN + RPN head on d_x NCHW fp32
 * [B,3,Hp,Wp] -> per level l (strides 4..64) NHWC fp32 [B,h_l,w_l,15]: 3 logits
 * (RegionProposalNetwork.log) then 3 x 4 deltas (.reg), rcnn.py:42-47. */
int vtf_rcnn_preprocess(vtf_rcnn_t h, const uint8_t* d_frames, int B, int H, int W, int64_t frame_stride,
                        int64_t row_stride, float* d_out);
int vtf_rcnn_rpn_heads(vtf_rcnn_t h, const float* d_x, int B, int Hp, int Wp, float* d_head0, float* d_head1,
                       float* d_head2, float* d_head3, float* d_head4);
/* RPN proposals of the last detect call (rcnn.py:82): host [n,5] (image, x1, y1, x2, y2). */
int vtf_rcnn_proposals(vtf_rcnn_t h, float* out, int64_t cap, int64_t* out_n);
/* RegionProposalNetwork.forward after the heads (rcnn.py:49-82: per-level top-1000, decode,
 * clamp, remove_small, batched_nms(0.7) by (image, level), top-1000 per image) on given head maps
 * (NHWC fp32 as vtf_rcnn_rpn_heads writes them) of a B x Hp x Wp input whose images are
 * h_used x w_used: host out [n,5] (image, x1, y1, x2, y2).  The integer path (top-k, NMS keep
 * sets) can so be checked on identical inputs. */
int vtf_rcnn_rpn_proposals(vtf_rcnn_t h, const float* d_head0, const float* d_head1, const float* d_head2,
                           const float* d_head3, const float* d_head4, int B, int Hp, int Wp, int h_used, int w_used,
                           float* out, int64_t cap, int64_t* out_n);
/* torchvision.ops.roi_align(fmap, rois, (7,7), spatial_scale, sampling_ratio=0, aligned=True)
 * as roi.py:31 calls it: d_fmap NHWC fp32 [N,H,W,C], d_rois fp32 [R,5] (image, x1, y1, x2, y2)
 * -> d_out NHWC fp32 [R,7,7,C]. */
int vtf_roi_align(const float* d_fmap, int N, int H, int W, int C, const float* d_rois, int64_t R,
                  float spatial_scale, float* d_out, void* hip_stream);
/* Timing of the body + FPN + RPN-head conv stack, as vtf_yolo_profile. */
int vtf_rcnn_profile(vtf_rcnn_t h, int enable, double* out_ms, int64_t* out_launches, double* out_flops,
                     int64_t* out_frames);

/* ---------------------------------------------------------------- grouping: K-means, scores
 * Replace the sklearn calls of cluster_faces (src/videotofaces/grouping.py:92-120):
 * KMeans(n_clusters=k, random_state, n_init='auto').fit(X), silhouette_score,
 * calinski_harabasz_score, davies_bouldin_score.  The host mirror (videotofaces/kmeans.py)
 * keeps sklearn's scalar control flow; these are its device passes.  All device arrays are
 * row-major, X float32 [N,D]. */
int vtf_group_create(int device, vtf_group_t* out);
int vtf_group_destroy(vtf_group_t h);
int vtf_group_set_stream(vtf_group_t h, void* hip_stream);
/* X.mean(axis=0), np.var(X, axis=0) (numpy's sequential fp32 axis-0 sums) and, if d_Xc is
 * not NULL, the centred copy X - mean (KMeans.fit, sklearn/cluster/_kmeans.py:1479-1481). */
int vtf_colstats(vtf_group_t h, const float* d_X, int64_t N, int64_t D, float* d_Xc, float* d_mean, float* d_var);
/* k-means++ distances (_kmeans.py:_kmeans_plusplus): d_out [T,N] = squared euclidean
 * distances of rows[0..T) (host int64 indices) to every row, sklearn's float64-upcast
 * formula rounded to fp32 and clipped at 0.  T <= 16. */
int vtf_sqdist_rows(vtf_group_t h, const float* d_X, int64_t N, int64_t D, const int64_t* rows, int T, float* d_out);
/* One Lloyd iteration (_k_means_lloyd.pyx lloyd_iter_chunked_dense): labels (in/out, int32)
 * from centers [k,D]; if d_sums: per-cluster sums [k,D] in sklearn's one-thread order
 * (sequential fp32 over the cluster's rows in row order, _update_chunk_dense) and weights
 * [k] (counts).  *out_changed = number of labels that changed.  k <= 64, N < 2^24. */
int vtf_kmeans_step(vtf_group_t h, const float* d_X, int64_t N, int64_t D, const float* d_centers, int k,
                    int32_t* d_labels, float* d_sums, float* d_weights, int64_t* out_changed);
/* _average_centers + _center_shift: sums -> centers in place, shift[k] = |new - old|. */
int vtf_kmeans_average(vtf_group_t h, float* d_sums, const float* d_weights, const float* d_centers_old, int k,
                       int64_t D, float* d_shift);
/* ((X - centers[labels])**2).sum(1) (empty-cluster relocation, _k_means_common.pyx). */
int vtf_center_dist(vtf_group_t h, const float* d_X, int64_t N, int64_t D, const float* d_centers,
                    const int32_t* d_labels, float* d_out);
/* pairwise_distances(X) euclidean [N,N] fp32 (float64-upcast, sqrt, zero diagonal). */
int vtf_pairwise_euclidean(vtf_group_t h, const float* d_X, int64_t N, int64_t D, float* d_out);
/* silhouette_samples from the distance matrix; labels encoded 0..k-1, freq int64 [k]. */
int vtf_silhouette_samples(vtf_group_t h, const float* d_D, int64_t N, const int32_t* d_labels, int k,
                           const int64_t* d_freq, float* d_sil);
/* silhouette_samples (sklearn/metrics/cluster/_unsupervised.py:203-315, called by
 * silhouette_score at grouping.py:105) of M label sets at once, for rows [row_begin, row_end)
 * only -- a rank's shard -- and without the N x N matrix (O(N*D) memory): d_labels uint8
 * [M][N] encoded 0..k_m-1, ks host int32 [M] (2 <= k_m, sum k_m <= 160 per call), freq host
 * int64 [sum k_m] (cluster sizes, set after set), d_sil float32 [M][row_end - row_begin].
 * Replaces vtf_pairwise_euclidean + vtf_silhouette_samples for the sweep. */
int vtf_silhouette_sweep(vtf_group_t h, const float* d_X, int64_t N, int64_t D, int64_t row_begin, int64_t row_end,
                         const uint8_t* d_labels, int M, const int32_t* ks, const int64_t* freq, float* d_sil);
/* Per-cluster float64 sums [k,D], sum of |x|^2 [k] and counts [k] (calinski_harabasz). */
int vtf_cluster_sums(vtf_group_t h, const float* d_X, int64_t N, int64_t D, const int32_t* d_labels, int k,
                     double* d_sums, double* d_sqnorm, int64_t* d_counts);
/* dsum[c] = sum over members of |x - centroid_c| in float64 (davies_bouldin intra_dists). */
int vtf_cluster_dist(vtf_group_t h, const float* d_X, int64_t N, int64_t D, const int32_t* d_labels, int k,
                     const double* d_centroids, double* d_dsum);

#ifdef __cplusplus
}
#endif
#endif /* VTF_H */
