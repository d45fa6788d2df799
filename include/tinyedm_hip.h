/* tinyedm_hip.h -- C ABI of libtinyedm_hip.so, the MI355X (gfx950) kernels behind the tinyedm hot path.
 *
 * The reference (YichengDWu/tinyedm) has no native code: every entry point below replaces an ATen op
 * call site of its Python hot path (cited as file:line relative to /root/reference/src/tinyedm) or the
 * autograd backward of one.  Conventions:
 *   - plain pointers + sizes only; every pointer is DEVICE memory owned by the caller (the one exception,
 *     edm_wgrad3_group's descriptor array, is HOST memory read during the call); compute entry points do no
 *     allocation and no host sync: work is enqueued on `stream` and is graph-capturable from the first call.
 *     The only allocating call is edm_init(device), made once per device before anything else.
 *   - activations: NHWC bf16, i.e. a row-major [pixels = B*H*W][channels] matrix of 16-bit brain floats.
 *   - per-(sample,channel) / parameter-side quantities: fp32.
 *   - return 0 on success, <0 on error (edm_last_error() holds the message, thread-local).
 */
#ifndef TINYEDM_HIP_H
#define TINYEDM_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* edm_stream_t; /* hipStream_t */

int edm_version(void);
const char* edm_last_error(void);
/* per-device constants (a 4 KiB page of zeros the LDS-DMA kernels point padding rows at): allocate once per device,
 * outside any stream capture; idempotent and thread-safe.  Every kernel that needs the page fails with -1 until then. */
int edm_init(int device);
/* hipGraph capture of these entry points: on ROCm 7.2 the runtime's default AQL-packet-capture path runs the first
 * replay that follows a hipStreamSynchronize / hipDeviceSynchronize with clobbered kernel arguments.  The library's
 * load-time constructor therefore sets DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 when the variable is unset (the runtime reads
 * it at its first HIP call: load this library before that).  Returns 1 when the environment holds the safe value. */
int edm_graph_replay_safe(void);
/* Per-step scalars of a hipGraph-captured training step.  By-value arguments are frozen into a graph at capture time;
 * entry points with a `dyn` parameter read these fields from DEVICE memory instead when dyn != NULL, so the host can
 * rewrite the 48-byte record (one small async copy) before every replay: step/seed feed the Philox streams of dropout
 * and the Diffuser (reference: torch RNG state advancing between steps), lr comes from the LambdaLR schedule
 * (edm.py:305-320), ema_beta from ema.py:137-140, bc1 = 1-b1^t and bc2sqrt = sqrt(1-b2^t) are Adam's bias corrections. */
typedef struct {
  unsigned step, seed_lo, seed_hi, reserved;
  float lr, ema_beta, grad_scale, bc1, bc2sqrt, pad[3];
} edm_step_params;

/* ---------------------------------------------------------------- convolution (networks.py:35-37: F.conv2d) */
/* Y[p,co] = alpha * sum_{tap,ci} X[p+off(tap),ci] * Wp[tap,co,ci] + beta * R[p,co].  taps in {1,9}; "same" padding.
 * Forward conv with the forward pack; input-gradient (dgrad) with the flipped/transposed pack.  R may be NULL. */
int edm_conv_igemm(const void* X, const void* Wp, void* Y, const void* R, float alpha, float beta, int B, int H,
                   int W, int Cin, int Cout, int taps, edm_stream_t stream);
/* second-generation kernel, same contract (LDS-DMA staging, 3-deep weight ring, 256x128 tile); returns -3 for shapes
 * it does not cover. */
int edm_conv_igemm_v2(const void* X, const void* Wp, void* Y, const void* R, float alpha, float beta, int B, int H,
                      int W, int Cin, int Cout, int taps, edm_stream_t stream);
/* the 3x3 kernel of the 32x32 / 16x16 layers ("static schedule": 512 pixels x 128 or 64 channels per workgroup, the
 * (tap, 2 channel-chunk) loop unrolled 18x, per-lane fragment addresses computed once, counted waits) on
 * v_mfma_f32_16x16x32_bf16; -3 for shapes it does not cover (taps != 9, Cin % 64 != 0, W > 64).  (Its 32x32x16
 * predecessor edm_conv_igemm_v4 and the tall-tile edm_conv_igemm_v3 were retired in round 4: no dispatch reached the
 * first, and the second ran one launch per step -- conv_in -- 10 us slower than edm_conv_igemm.) */
int edm_conv_igemm_v6(const void* X, const void* Wp, void* Y, const void* R, float alpha, float beta, int B, int H,
                      int W, int Cin, int Cout, int taps, edm_stream_t stream);
/* small feature maps (8x8 layers; W <= 16, Cin % 256 == 0), 3x3 only: 128x64 tile whose reduction dimension is split
 * over the four waves of the workgroup (private LDS regions, no barrier in the main loop, fixed-order LDS reduction);
 * -3 for shapes it does not cover */
int edm_conv_igemm_s(const void* X, const void* Wp, void* Y, const void* R, float alpha, float beta, int B, int H,
                     int W, int Cin, int Cout, int taps, edm_stream_t stream);
/* Which of the four kernels above runs a convolution of this shape: host logic only (no device call, no edm_init needed),
 * the plan the fused entry points below launch from and the Python side asks for.  Returns the kernel id of
 * edm_conv_igemm_o in the low byte (1 edm_conv_igemm, 2 _v2, 5 _s, 6 _v6) and, for kernel 6, the channel width of its
 * tiles (128 or 64) in the next byte.  force: 0 = chosen per shape; 1 / 2 / 5 / 6 = that generation where it covers the
 * shape, kernel 1 where it does not (EDM_IGEMM of the Python side; the fused entry points always plan with 0). */
int edm_conv_plan(int B, int H, int W, int Cin, int Cout, int taps, int force);
/* Same operation with an OUTPUT DESCRIPTOR -- how torch.cat((input, skip * gate)) (networks.py:311) and its backward stop
 * being copies: Y rows have stride ldY elements (0 = Cout: Y may be the left column block of the next block's
 * concatenated operand); Ysilu (optional) receives mp_silu(Y) at the same offsets of a second buffer with the same stride
 * (the operand of that block's first 3x3 conv, networks.py:315); Yb (optional): output channels >= split go to
 * Yb[pixel * ldYb + channel - split] (the 1x1 dgrad that produces d loss / d cat writes d loss / d input and the raw
 * gradient of the gated skip to the two tensors their consumers read).  kernel: which generation runs (1 edm_conv_igemm,
 * 2 _v2, 5 _s, 6 _v6; -3 = shape not covered by it).  R stays contiguous [pixels][Cout].
 * wfrag != 0: Wp is a FRAGMENT-MAJOR pack (edm_weight_prep_multi, bits 8 / 9 of a record's taps field) -- the layout the
 * 8x8 layers' kernel loads with coalesced 1-KiB instructions straight into MFMA operand registers; kernel 5 only.  The
 * three fused 3x3 entry points below take the same flag (then they run kernel 5 whatever the shape heuristics say). */
int edm_conv_igemm_o(const void* X, const void* Wp, void* Y, long ldY, void* Ysilu, void* Yb, long ldYb, int split,
                     const void* R, float alpha, float beta, int B, int H, int W, int Cin, int Cout, int taps, int kernel,
                     int wfrag, edm_stream_t stream);
/* Folded skip projection (round 6): Y = alpha3 * conv3x3(X, Wp) + alpha1 * conv1x1(X2, W2p) in ONE launch of the
 * static-schedule 3x3 kernel -- the decoder block's conv_1x1(cat) (networks.py:313) as a second reduction behind the nine taps
 * of the block's second 3x3 conv (networks.py:325-327), whose residual it was.  X2 [pixels][ldX2] (first C2 channels read),
 * W2p [Cout][C2] = the 1x1 conv's forward pack; Y / ldY / Ysilu as edm_conv_igemm_o.  edm_conv3x3_fold_supported() -> 1 / 0;
 * the entry point returns -3 for shapes it does not cover (the caller keeps the two launches). */
int edm_conv3x3_fold_supported(int B, int H, int W, int Cin, int Cout, int C2);
int edm_conv3x3_fold(const void* X, const void* Wp, const void* X2, long ldX2, const void* W2p, int C2, void* Y, long ldY,
                     void* Ysilu, float alpha3, float alpha1, int B, int H, int W, int Cin, int Cout, edm_stream_t stream);
/* first 3x3 conv of a block with the embedding modulation fused into its epilogue (networks.py:253-260 / 317-324):
 * Y = conv3x3(X) (bf16, may be NULL in eval), Y2 = dropout(mp_silu(Y * (lin[b,:]*gain + 1))) -- bit-identical to
 * edm_mod_silu_drop_fwd applied to Y (same Philox counters), so edm_mod_silu_drop_bwd serves as its backward. */
int edm_conv3x3_mod(const void* X, const void* Wp, void* Y, void* Y2, const float* lin, long lin_stride,
                    const float* gain, float pdrop, unsigned long long seed, unsigned sub, unsigned step, int mark_dropped,
                    int B, int H, int W, int Cin, int Cout, const void* dyn, int wfrag, edm_stream_t stream);
/* backward counterpart: dgrad of the block's second 3x3 conv (ga = alpha*conv3x3(dY, Wd), never written) with the
 * modulation backward in the epilogue: GR = ga*keep*mp_silu'(u*m)*m, gm[b,c] += sum_px ga*keep*mp_silu'(u*m)*u (gm
 * zero-filled fp32, rows of gm_stride floats, 0 = Cout); finish with edm_mod_finish, or -- when gm is a column slice of a
 * buffer shared by all blocks -- with ONE edm_mod_finish_multi at the end of the backward pass.  -3 when H*W % 32 != 0
 * (use the separate kernels).  mark_dropped (forward) writes NaN into the elements of Y (= U) the dropout removed; with
 * u_marked (backward) the mask is read back from those NaNs instead of regenerating the Philox stream (a third of the
 * backward epilogue's vector-ALU work). */
int edm_conv3x3_modbwd(const void* dY, const void* Wd, float alpha, const void* U, const float* lin, long lin_stride,
                       const float* gain, void* GR, float* gm, long gm_stride, float pdrop, unsigned long long seed,
                       unsigned sub, unsigned step, int u_marked, int B, int H, int W, int Cin, int Cout, const void* dyn,
                       int wfrag, edm_stream_t stream);
/* dgrad of a block's first 3x3 conv with the mp_silu backward of the block input in its epilogue
 * (g = conv3x3(dY, Wd) never written): GX = mp_silu'(Xpre)*g + add_scale*ADD (ADD may be NULL). */
int edm_conv3x3_silubwd(const void* dY, const void* Wd, const void* Xpre, const void* ADD, float add_scale, void* GX,
                        int B, int H, int W, int Cin, int Cout, int wfrag, edm_stream_t stream);
int edm_mod_finish(const float* gm, const float* lin, long lin_stride, const float* gain, float* glin, long glin_stride,
                   float* ggain, int B, int C, edm_stream_t stream);
/* every block's finish in one launch: gm_all / lin_all / glin_all are [B][stride] fp32, items a DEVICE array of
 * {const float* gain; float* ggain; int col0, C;}: glin[:, col0:col0+C] += gm * *gain, *ggain += sum gm * lin */
int edm_mod_finish_multi(const float* gm_all, const float* lin_all, float* glin_all, long stride, const void* items_dev,
                         int n_items, int B, edm_stream_t stream);
/* weight gradient: slabs[s,tap,co,ci] (fp32, nsplit = edm_conv_wgrad_nsplit(...)) partial sums over pixels; LDS-DMA staging,
 * rolling X window; Cin, Cout % 32 == 0; -3 = not covered (3x3 with W > 126).  (The first-generation edm_conv_wgrad was retired
 * in round 6: no default dispatch reached it.) */
int edm_conv_wgrad_nsplit(int B, int H, int W, int Cin, int Cout, int taps);
int edm_conv_wgrad_v2(const void* X, const void* dY, float* slabs, int B, int H, int W, int Cin, int Cout, int taps,
                      int nsplit, edm_stream_t stream);
/* 1x1 layers (networks.py:21-38 with kernel_size 1: skip projections, attention qkv/out): 256x128-output tiles,
 * slabs fp32 [nsplit][Cout][Cin] with nsplit = edm_conv_wgrad_1x1_nsplit(npix, Cin, Cout); Cin, Cout % 32 == 0. */
int edm_conv_wgrad_1x1_nsplit(long npix, int Cin, int Cout);
int edm_conv_wgrad_1x1(const void* X, const void* dY, float* slabs, long npix, int Cin, int Cout, int nsplit,
                       edm_stream_t stream);
/* up to 16 1x1 layers in ONE launch (their (tile, split) workgroups laid end to end in one grid); `items` is a HOST array
 * read during the call */
typedef struct {
  const void* X;   /* bf16 [npix][Cin] */
  const void* dY;  /* bf16 [npix][Cout] */
  float* slabs;    /* fp32 [nsplit][Cout][Cin], nsplit = edm_conv_wgrad_1x1_nsplit_grouped(npix, Cin, Cout) */
  long npix;
  int Cin, Cout, nsplit, pad;
} edm_wgrad1_item;
int edm_conv_wgrad_1x1_nsplit_grouped(long npix, int Cin, int Cout);
/* LAUNCH TABLES (round 4): the three grouped entry points below keep their per-layer table in DEVICE memory -- no kernel
 * takes a multi-KB by-value argument (a suspect of the hipGraph corruption of round 2).  The caller passes
 * table_host (PINNED host memory) and table_dev (device memory), each of at least edm_*_table_bytes() bytes: the call
 * fills table_host, issues ONE stream-ordered copy to table_dev (a memcpy node when the stream is being captured) and
 * launches with the device pointer.  table_host must stay valid and unmodified until that copy has executed (for a
 * captured stream: for the life of the graph), table_dev until the kernels have.  defer_upload != 0: the call only fills
 * table_host (any host memory) and launches; the CALLER copies table_host to table_dev before the launch can execute -- for
 * a stream capture once, after the capture has ended, instead of a copy node that every replay would run again. */
long edm_conv_wgrad_1x1_group_table_bytes(void);
int edm_conv_wgrad_1x1_group(const edm_wgrad1_item* items, int n, void* table_host, void* table_dev, int defer_upload,
                             edm_stream_t stream);
/* third generation, 3x3 layers, a GROUP of layers per call (autograd wgrad of networks.py:35-37 + the projection of
 * networks.py:32-36's normalisation): the reduction dimension of all layers is laid end to end and cut into equal
 * ranges, one per workgroup (128x64x9 tile, one wave per SIMD); partial tiles go to `workspace`; a second launch sums
 * each weight row's partials, projects through w_hat = w/(eps + |w|/sqrt(n))/sqrt(n) and writes (accumulate=0) or
 * accumulates (1) grad.  `items` is a HOST array read during the call; <= edm_wgrad3_max_layers() (48) layers, all with W <= 62 or all with
 * 62 < W <= 126; Cin, Cout % 32 == 0.  workspace >= edm_wgrad3_workspace(items, n) bytes (-1 on bad arguments). */
typedef struct {
  const void* X;    /* bf16 [B*H*W][Cin]  layer input */
  const void* dY;   /* bf16 [B*H*W][Cout] gradient of the layer output */
  const float* w;   /* fp32 master weight [Cout][I][3][3] */
  float* grad;      /* fp32 gradient of w, same layout */
  const int* perm;  /* packed output row -> master row, or NULL */
  int B, H, W, Cin, Cout, I; /* I <= Cin: input channels of w (X may be zero-padded to Cin) */
  float scale;      /* gradient scale folded in before the projection */
  int accumulate;
} edm_wgrad3_item;
long edm_wgrad3_workspace(const edm_wgrad3_item* items, int n);
long edm_wgrad3_table_bytes(void);
int edm_wgrad3_max_layers(void);
int edm_wgrad3_group(const edm_wgrad3_item* items, int n, void* workspace, long workspace_bytes, void* table_host,
                     void* table_dev, int defer_upload, edm_stream_t stream);
/* apply form: the finish launch runs edm_adam_ema's update (g = projected gradient * grad_scale) on the weight rows it
 * holds instead of writing their gradient -- w, m, v and ema rows are rewritten, `grad` is not touched for them.  opt[k]:
 * the m / v / ema (nullable) tensors of layer k, laid out like its w; dyn: the DEVICE edm_step_params record, required: lr,
 * ema_beta, grad_scale and the bias corrections are read at run time; health: as edm_adam_ema.  A layer whose rows (I * 9 floats)
 * exceed the kernel's register prefetch (7168) keeps the plain finish into `grad`.  fused_out (HOST, n ints): 1 = layer k
 * was updated here, 0 = its gradient is in `grad`.  The launch table takes edm_wgrad3_apply_table_bytes(). */
typedef struct {
  float* m;
  float* v;
  float* ema;
} edm_wgrad3_opt;
long edm_wgrad3_apply_table_bytes(void);
int edm_wgrad3_group_apply(const edm_wgrad3_item* items, int n, void* workspace, long workspace_bytes, void* table_host,
                           void* table_dev, int defer_upload, const edm_wgrad3_opt* opt, const void* dyn, float b1,
                           float b2, float eps, unsigned* health, int* fused_out, edm_stream_t stream);

/* ---------------------------------------------------------------- weights (networks.py:17-19, 32-36, 55-59) */
/* forced weight normalisation (in place when normalize_inplace) + effective weight w/(eps+|w|/sqrt(n))/sqrt(n),
 * written as bf16 forward pack [taps,O,Ipad], bf16 dgrad pack [taps,I,O] (taps flipped) and/or fp32 [O,I*taps]. */
int edm_weight_prep(float* w, int O, int I, int taps, int Ipad, void* wp_fwd, void* wp_dgrad, float* w_hat,
                    const int* perm, int normalize_inplace, edm_stream_t stream);
/* multi-tensor form: one launch for every weight of a network.  descs = device array of 64-byte records
 * {float* w; bf16* fwd; bf16* dgrad; float* hat; const int* perm; int O, I, taps, Ipad, row0, rb;}; groups = device
 * int32 [n_groups][2] = (record index, first packed row): one workgroup prepares <= rb consecutive rows of a record
 * through an LDS tile of rb*I*taps bf16 (lds_bytes = the largest such tile, <= 128 KiB). */
int edm_weight_prep_multi(const void* descs, const int* groups, int n_groups, int lds_bytes, int normalize_inplace,
                          edm_stream_t stream);
/* reduce split-K slabs and project through the normalisation -> gradient of the fp32 master weight [O,I,taps]. */
int edm_wgrad_finish(const float* slabs, int S, const float* w, float* grad, const int* perm, int O, int I, int Ipad,
                     int taps, float scale, int accumulate, edm_stream_t stream);

/* the same for up to 40 tensors in ONE launch (`items` is a HOST array read during the call) */
typedef struct {
  const float* slabs; /* fp32 [S][taps][O][Ipad] */
  const float* w;     /* fp32 master weight [O][I][taps] */
  float* grad;        /* fp32 gradient, same layout */
  const int* perm;    /* or NULL */
  int S, O, I, Ipad, taps;
  float scale;
  int accumulate;
} edm_finish_item;
long edm_wgrad_finish_multi_table_bytes(void);
int edm_wgrad_finish_multi(const edm_finish_item* items, int n, void* table_host, void* table_dev, int defer_upload,
                           edm_stream_t stream);

/* ---------------------------------------------------------------- attention (networks.py:194-202) */
/* qkv [B*N,3C] channel order [head][q|k|v][d]; q,k,v pixel-normalised over d; softmax(qk^T/sqrt(d)) v. d = 64, N<=256 */
int edm_attention_fwd(const void* qkv, void* y, int B, int N, int C, int heads, edm_stream_t stream);
int edm_attention_bwd(const void* qkv, const void* y, const void* gy, void* gqkv, int B, int N, int C, int heads,
                      edm_stream_t stream);

/* The same attention for any number of tokens N >= 1 (csrc/attention_long.hip; networks.py:194-202 at whatever resolution
 * the level has): key tiles of 64 and a fixed-offset softmax p = exp(s - sqrt(d)) -- pixel-normalised q, k bound every
 * logit by sqrt(d), so there is no running maximum.  Head dims 64, 32, 128, 144, 192.
 * edm_attention_long_supported: 1 / 0 (head_dim built, N >= 1). */
int edm_attention_long_supported(int N, int C, int heads);
/* networks.py:194-202.  stat [B, heads, N] fp32 = the rows' log-sum-exp sqrt(d) + log sum p, kept for the backward; may be
 * NULL in evaluation. */
int edm_attention_long_fwd(const void* qkv, void* y, float* stat, int B, int N, int C, int heads, edm_stream_t stream);
/* autograd of networks.py:194-202: y, stat = the forward's outputs; work = B*heads*N floats (delta = <dO, y>, written by the
 * query-major kernel, read by the key-major one).  No atomics: gqkv is bit-reproducible. */
int edm_attention_long_bwd(const void* qkv, const void* y, const void* gy, const float* stat, void* gqkv, float* work,
                           int B, int N, int C, int heads, edm_stream_t stream);

/* CosineAttention with the qkv projection inside the attention kernel (csrc/attention_fused.hip, round 5; replaces
 * networks.py:193-202 = qkv_conv -> view -> pixel_norm -> scaled_dot_product_attention as ONE launch; the qkv tensor never
 * exists in HBM).  x [B*N, C] bf16 tokens, Wqkv [3C, C] bf16 = the qkv conv's forward pack (rows in [head][q|k|v][d] order),
 * y [B*N, C] bf16, stat [B, heads, N] fp32 (softmax normaliser, kept for the backward; may be NULL in evaluation).
 * Covered: C = 256, 4 heads (head_dim 64), 33..256 tokens (edm_attention_qkv_supported); heads_per_wg 0 = default. */
int edm_attention_qkv_supported(int N, int C, int heads);
int edm_attention_qkv_fwd(const void* x, const void* Wqkv, void* y, void* stat, int B, int N, int C, int heads,
                          int heads_per_wg, edm_stream_t stream);
/* its backward (autograd of networks.py:193-205 up to the projections' own GEMMs): gqkv [B*N, 3C] bf16, packed channel order,
 * = d loss / d qkv_conv(x) from gout = d loss / d out_conv(y) [B*N, C].  dO = alpha * gout . W_out is formed inside from
 * Wd_out = the out conv's dgrad pack [C, C] (alpha = the mp_add coefficient of the attention branch); q, k, v are recomputed
 * from x and Wqkv; y, stat = the forward's outputs.  The callers' remaining launches: the qkv conv's dgrad (gx) and the two
 * weight gradients.  heads_per_wg: 0 or 1 (the backward runs one head per workgroup; anything else is refused). */
int edm_attention_qkv_bwd(const void* x, const void* y, const void* gout, const void* stat, const void* Wqkv,
                          const void* Wd_out, void* gqkv, float alpha, int B, int N, int C, int heads, int heads_per_wg,
                          edm_stream_t stream);

/* ---------------------------------------------------------------- per-pixel / elementwise */
/* pixel_norm over C + mp_silu (networks.py:9-14, 83-84, 249-252); dsave[p] = eps + |x_p|/sqrt(C) */
int edm_pixelnorm_silu_fwd(const void* x, void* xn, void* a, float* dsave, long P, int C, edm_stream_t stream);
/* gadd (optional, bf16 like gx): added to the result -- the gradient reaching the same tensor along the U-Net skip, which
 * autograd would otherwise sum with a separate add (networks.py:592-600: the encoder output feeds the next block AND a
 * decoder block) */
int edm_pixelnorm_silu_bwd(const void* xn, const float* dsave, const void* gxn, float gxn_scale, const void* ga,
                           const void* gadd, void* gx, long P, int C, edm_stream_t stream);
/* round 6: the same pair with the 2x2 average pool of an EncD block folded in (networks.py:246-252, blocks without a 1x1
 * conv): x / gx / gadd are (B, 2 Hp, 2 Wp, C) -- the tensor BEFORE the pool --, xn / a / dsave / gxn / ga (B, Hp, Wp, C); the
 * pooled tensor is never written.  Bit-identical to edm_pool2(0.25) + edm_pixelnorm_silu_fwd and to edm_pixelnorm_silu_bwd +
 * edm_up2(0.25, add = gadd).  C <= 1024. */
int edm_pool_pixelnorm_silu_fwd(const void* x, void* xn, void* a, float* dsave, int B, int Hp, int Wp, int C,
                                edm_stream_t stream);
int edm_pool_pixelnorm_silu_bwd(const void* xn, const float* dsave, const void* gxn, float gxn_scale, const void* ga,
                                const void* gadd, void* gx, int B, int Hp, int Wp, int C, edm_stream_t stream);
/* mp_silu (networks.py:316) and its backward: gx = mp_silu'(x)*ga + extra_scale*gextra */
int edm_silu_fwd(const void* x, void* a, long n, edm_stream_t stream);
int edm_silu_bwd(const void* x, const void* ga, const void* gextra, float extra_scale, void* gx, long n,
                 edm_stream_t stream);
/* out = alpha*a + beta*b (mp_add, networks.py:87-88) */
int edm_axpby(const void* a, float alpha, const void* b, float beta, void* out, long n, edm_stream_t stream);
/* a = dropout(mp_silu(r * (lin*gain + 1)))  (networks.py:255-260 / 319-324); Philox mask from (seed, sub, step) */
int edm_mod_silu_drop_fwd(const void* r, const float* lin, long lin_stride, const float* gain, void* a, int B, int HW,
                          int C, float pdrop, unsigned long long seed, unsigned sub, unsigned step, const void* dyn,
                          edm_stream_t stream);
int edm_mod_silu_drop_bwd(const void* r, const float* lin, long lin_stride, const float* gain, const void* ga, void* gr,
                          float* gm, float* glin, long glin_stride, float* ggain, int B, int HW, int C, float pdrop,
                          unsigned long long seed, unsigned sub, unsigned step, const void* dyn, edm_stream_t stream);
/* its first half alone: gr, and the raw modulation gradient accumulated into gm (zero-filled fp32, rows of gm_stride floats:
 * a column slice of the buffer all blocks share) -- finished for every block by ONE edm_mod_finish_multi (the form
 * edm_conv3x3_modbwd takes with a shared buffer, for maps whose H*W is no multiple of 32, which that entry refuses) */
int edm_mod_silu_drop_bwd_raw(const void* r, const float* lin, long lin_stride, const float* gain, const void* ga, void* gr,
                              float* gm, long gm_stride, int B, int HW, int C, float pdrop, unsigned long long seed,
                              unsigned sub, unsigned step, const void* dyn, edm_stream_t stream);
int edm_dropout_mask(unsigned char* mask, long n, float pdrop, unsigned long long seed, unsigned sub, unsigned step,
                     edm_stream_t stream);
/* 2x2 average pool / nearest-exact x2 (networks.py:80, 72); H,W = OUTPUT dims; scale folds the backward factors */
int edm_pool2(const void* x, void* y, int B, int Hout, int Wout, int C, float scale, edm_stream_t stream);
/* up2: y = scale * up(x) + add (add optional, same shape as y: see edm_pixelnorm_silu_bwd's gadd) */
int edm_up2(const void* x, const void* add, void* y, int B, int Hout, int Wout, int C, float scale, edm_stream_t stream);
/* DecU blocks (networks.py:312-316): y = nearest-exact x2 of x and a = mp_silu(y) in one pass (== edm_up2 + edm_silu_fwd) */
int edm_up2_silu(const void* x, void* y, void* a, int B, int Hout, int Wout, int C, edm_stream_t stream);
/* out[b,c] = scale * sum_hw x[b,hw,c] (* y[b,hw,c])  -- ScaleLong mean (networks.py:116) and its gate gradient;
 * written, not accumulated, in a fixed summation order (bit-reproducible) */
int edm_reduce_hw(const void* x, long x_stride, const void* y, long y_stride, float* out, int B, int HW, int C,
                  float scale, edm_stream_t stream);
/* ScaleLong gate MLP (networks.py:112-118), fp32, per sample */
int edm_scalelong_fwd(const float* mean, const float* W1h, const float* W2h, float* gate, float* z1save, int B, int C,
                      int R, edm_stream_t stream);
int edm_scalelong_bwd(const float* mean, const float* W1h, const float* W2h, const float* gate, const float* z1save,
                      const float* ggate, float* gmean, float* gW1h, float* gW2h, int B, int C, int R,
                      edm_stream_t stream);
/* The two steps above in ONE launch per direction (one workgroup per sample: mean over H*W in a fixed order, then the
 * sample's gate MLP from LDS).  fwd: skip [B*HW][C] bf16 -> mean, gate [B][C], z1save [B][R].  bwd: channels
 * [c_off, c_off+C) of gcat (rows of gcat_stride elements) are d loss / d (skip*gate); ggate = sum_hw gcat*skip is formed
 * and consumed in place; gmean, gW1h [R][C+1] and gW2h [C][R] are written (the weight gradients by a second small launch
 * that sums the per-sample outer products over the batch in a fixed order); ws: [B][C + 2R] floats of scratch. */
int edm_skip_gate_fwd(const void* skip, const float* W1h, const float* W2h, float* mean, float* gate, float* z1save,
                      int B, int HW, int C, int R, edm_stream_t stream);
int edm_skip_gate_bwd(const void* gcat, long gcat_stride, int c_off, const void* skip, const float* mean,
                      const float* W1h, const float* W2h, const float* gate, const float* z1save, float* gmean,
                      float* gW1h, float* gW2h, float* ws, int B, int HW, int C, int R, edm_stream_t stream);
/* round 6: gW1h == gW2h == NULL in edm_skip_gate_bwd skips its second launch (the batch sums of the weight gradients); the
 * caller then runs it ONCE for all the gates of a backward pass (<= 32): items[k] = {ws, mean of gate k, gW1h, gW2h (written),
 * B, C, R}.  Launch-table contract as edm_wgrad_finish_multi (table_host / table_dev / defer_upload). */
typedef struct {
  const float* ws;
  const float* mean;
  float* gW1h;
  float* gW2h;
  int B, C, R, pad;
} edm_skip_gate_wgrad_item;
long edm_skip_gate_wgrad_multi_table_bytes(void);
int edm_skip_gate_wgrad_multi(const edm_skip_gate_wgrad_item* items, int n, void* table_host, void* table_dev,
                              int defer_upload, edm_stream_t stream);
/* round 6: edm_skip_gate_fwd for up to 32 skip tensors of ONE channel count in one launch (the U-Net's skips all exist when
 * the encoder ends; one workgroup per (tensor, sample): a launch that fills the chip instead of nine half-empty ones on the
 * decoder's critical chain).  Same values as the per-tensor entry point.  Launch-table contract as above. */
typedef struct {
  const void* skip;     /* bf16 [B*HW][C] */
  const float* W1h;     /* [R][C+1] */
  const float* W2h;     /* [C][R] */
  float* mean;          /* [B][C]  written */
  float* gate;          /* [B][C]  written */
  float* z1save;        /* [B][R]  written */
  void* cat;            /* optional: bf16 rows of Ci + C elements; columns [Ci, Ci + C) receive skip * gate (edm_skip_half_fwd's */
  void* silu_out;       /* work, done by the workgroup that just reduced the sample) and, if given, mp_silu of it here */
  int B, HW, C, R, Ci, pad;
} edm_skip_gate_fwd_item;
long edm_skip_gate_fwd_multi_table_bytes(void);
int edm_skip_gate_fwd_multi(const edm_skip_gate_fwd_item* items, int n, void* table_host, void* table_dev, int defer_upload,
                            edm_stream_t stream);
/* ... and the backward of those gates, deferred: nothing on the backward's critical chain needs a gate's gmean (it only feeds
 * the gradient of the U-Net skip, which the encoder's backward consumes), so the decoder blocks queue and the last one
 * launches (a) edm_skip_gate_bwd_multi = the first launch of edm_skip_gate_bwd (gmean, ws written; weight gradients by
 * edm_skip_gate_wgrad_multi as before) for all gates of one channel count, (b) edm_skip_half_bwd_multi = edm_skip_half_bwd for
 * all their tensors.  Tables of edm_skip_gate_bwd_multi_table_bytes() bytes. */
typedef struct {
  const void* gcat;     /* bf16 rows of gcat_stride elements; channels [c_off, c_off + C) = d loss / d (skip * gate) */
  long gcat_stride;
  const void* skip;     /* bf16 [B*HW][C] */
  const float* W1h;
  const float* W2h;
  const float* gate;
  const float* z1save;
  float* gmean;         /* [B][C]       written */
  float* ws;            /* [B][C + 2R]  written */
  void* gskip;          /* optional: bf16 [B*HW][C] written = gcat[:, c_off:c_off+C] * gate + gmean / HW (edm_skip_half_bwd's work) */
  int c_off, B, HW, C, R, pad;
} edm_skip_gate_bwd_item;
typedef struct {
  const void* gcs;      /* bf16 [B*HW][Cs] */
  const float* gate;
  const float* gmean;
  void* gskip;          /* bf16 [B*HW][Cs]  written: gcs * gate + gmean / HW */
  int B, HW, Cs, pad;
} edm_skip_half_bwd_item;
long edm_skip_gate_bwd_multi_table_bytes(void);
int edm_skip_gate_bwd_multi(const edm_skip_gate_bwd_item* items, int n, void* table_host, void* table_dev, int defer_upload,
                            edm_stream_t stream);
int edm_skip_half_bwd_multi(const edm_skip_half_bwd_item* items, int n, void* table_host, void* table_dev, int defer_upload,
                            edm_stream_t stream);
/* cat = [inp, skip*gate] (networks.py:311) and backward */
int edm_concat_gate_fwd(const void* inp, const void* skip, const float* gate, void* cat, void* silu_out, int B, int HW,
                        int Ci, int Cs, edm_stream_t stream);
int edm_concat_gate_bwd(const void* gcat, const float* gate, const float* gmean, void* ginp, void* gskip, int B,
                        int HW, int Ci, int Cs, edm_stream_t stream);
/* The skip half alone (the input half is written by the producer of `input` through edm_conv_igemm_o):
 * cat[b,p,Ci:] = skip*gate, silu_out[b,p,Ci:] = mp_silu(of it) (rows of Ci + Cs elements; silu_out may be NULL); and
 * gskip = gcs*gate + gmean/HW from the skip half gcs [B*HW][Cs] of d loss / d cat. */
int edm_skip_half_fwd(const void* skip, const float* gate, void* cat, void* silu_out, int B, int HW, int Ci, int Cs,
                      edm_stream_t stream);
int edm_skip_half_bwd(const void* gcs, const float* gate, const float* gmean, void* gskip, int B, int HW, int Cs,
                      edm_stream_t stream);

/* ---------------------------------------------------------------- EDM preconditioning (networks.py:578-587, 602-603) */
/* out[b,h,w,:] = [c_in(b)*noisy[b,:,h,w], 1, 0...] (bf16, CP channels); sigma_stride 0 = one scalar sigma */
int edm_precond_in(const float* noisy, const float* sigma, int sigma_stride, float sigma_data, void* out, int B,
                   int Cimg, int HW, int CP, edm_stream_t stream);
/* The input gradient of the denoiser (reference networks.py:584-587, 602-603; conv_in_dgrad.hip): conv_in's 3x3 dgrad into
 * the Cimg image channels with the preconditioning folded in,
 *   gx[b,c,h,w] = c_in(b) * sum_{ky,kx,co} gy[b, h+1-ky, w+1-kx, co] * w^[co,c,ky,kx]  (zero outside the map)
 *               + c_skip(b) * gD[b,c,h,w]                                               (gD nullable: the term is absent)
 * gy: bf16 NHWC [B,H,W,C0], the gradient of conv_in's output; gx, gD: fp32 NCHW [B,Cimg,H,W], 1 <= Cimg <= 8; the constant
 * ones channel gets no gradient.  wpack: fp32 [C0][NT], NT = edm_conv_in_dgrad_pack_cols(Cimg) = 9*Cimg rounded up to 4,
 * wpack[co][(ky*3+kx)*Cimg + c] = w^[co,c,ky,kx] (the bf16-rounded forward operand), padding columns zero, 16-byte aligned.
 * fp32 accumulation in a fixed order (co ascending per tap, then the taps ky, kx ascending); the c_skip product is rounded on
 * its own, so gy = 0 returns c_skip * gD bit for bit; a sample's result does not depend on B.  gy may be 2-byte aligned
 * (16-byte pieces when it is 16-byte aligned and C0 % 8 == 0, same bits otherwise).  sigma_stride 0 = one scalar sigma.
 * EDM_ERR_UNSUPPORTED when three rows of W pixels do not fit the LDS table. */
int edm_conv_in_dgrad_pack_cols(int Cimg);
int edm_conv_in_dgrad(const void* gy, const float* wpack, const float* gD, const float* sigma, int sigma_stride,
                      float sigma_data, float* gx, int B, int Cimg, int H, int W, int C0, edm_stream_t stream);
/* D = conv_out(x)*gain_out*c_out + noisy*c_skip (fp32 NCHW); Fraw = conv_out(x) saved for the backward */
int edm_conv_out_fwd(const void* x, const float* w_hat, const float* gain_out, const float* noisy, const float* sigma,
                     int sigma_stride, float sigma_data, float* D, float* Fraw, int B, int HW, int C, int Co,
                     edm_stream_t stream);
int edm_conv_out_bwd(const void* x, const float* w_hat, const float* gain_out, const float* Fraw, const float* dD,
                     const float* sigma, int sigma_stride, float sigma_data, void* gx, float* gw_hat, float* ggain,
                     int B, int HW, int C, int Co, edm_stream_t stream);

/* ---------------------------------------------------------------- the output end in factored form (csrc/tail_lowrank.hip)
 * conv_out's input gradient g_h = dF . Wout has rank Co <= 8 per pixel; the last decoder block's second 3x3 conv takes its
 * dgrad and its weight gradient from dF (fp32 NCHW [B, Co, H, W]) instead of the C-channel g_h.  t = 3 ky + kx,
 * d(t) = (ky - 1, kx - 1); zero padding; any H, W; C % 8 == 0.  (edm_conv_out_bwd with gw_hat == NULL writes gx only.) */
/* dF = dD * c_out(b) * gain_out; aux (nullable) = dD * c_out(b) * Fraw, whose sum is d loss / d gain_out */
int edm_lowrank_df(const float* dD, const float* Fraw, const float* gain_out, const float* sigma, int sigma_stride,
                   float sigma_data, float* dF, float* aux, int B, int Co, int HW, edm_stream_t stream);
/* ga2 (bf16 NHWC, nullable when r1 is given) = scale * sum_t sum_o dF[p - d(t), o] * Wc[o][t][c], Wc fp32 [Co][9][C].
 * r1 != NULL: edm_conv3x3_modbwd's epilogue on ga2 in registers (gr, raw modulation sums += into zero-filled gm rows). */
int edm_lowrank_dgrad3x3(const float* dF, const float* Wc, float scale, void* ga2, const void* r1, const float* lin,
                         long lin_stride, const float* gain, void* gr, float* gm, long gm_stride, float pdrop,
                         unsigned long long seed, unsigned sub, unsigned step, int u_marked, int B, int H, int W, int C,
                         int Co, const void* dyn, edm_stream_t stream);
/* G (fp32 [Co][taps][C], overwritten) = sum_p dF[p, o] * X[p + d(t), c]; X bf16 NHWC, taps 1 or 9.  Deterministic (workgroup
 * partials in ws, edm_lowrank_wgrad_workspace(C, Co, taps) floats, added in a fixed order; no atomics).
 * aux (nullable, like dF): *aux_out += sum of aux. */
long edm_lowrank_wgrad_workspace(int C, int Co, int taps);
/* 1 when the LDS tables of edm_lowrank_wgrad(taps) -- and, taps == 9, of the fused edm_lowrank_dgrad3x3 -- fit for maps of
 * width W with C channels (60 KB: e.g. Co <= 5 at C = 256); the entry points refuse other shapes.  Host logic only. */
int edm_lowrank_supported(int C, int Co, int W, int taps);
int edm_lowrank_wgrad(const float* dF, const void* X, int taps, const float* aux, float* G, float* aux_out, float* ws,
                      long ws_floats, int B, int H, int W, int C, int Co, edm_stream_t stream);
/* Wc[o][t][i] = sum_c Wout_hat[o, c] * float(wd[taps - 1 - t][i][c]): wd = the plain bf16 dgrad pack [taps][I][O] of the conv */
int edm_lowrank_expand_wc(const float* wout_hat, const void* wd, float* Wc, int Co, int O, int I, int taps,
                          edm_stream_t stream);
/* slab[t][c][i] = scale * sum_o Wout_hat[o, c] * G[o][t][i]: one slab [1][taps][O][Ipad] for edm_wgrad_finish(_multi) */
int edm_lowrank_expand_slab(const float* wout_hat, const float* G, float* slab, float scale, int Co, int O, int I,
                            int Ipad, int taps, edm_stream_t stream);
/* The forward side of the same algebra: the block ends in h = sb * conv3x3(a2, W2) + sa * conv1x1(cat, W1) and conv_out
 * reads nothing else, so F = Wout . h = sb * conv3x3(a2, Wc) + sa * cat . Wp with Wp = Wout . W1 (fp32 [Co][Cc];
 * edm_lowrank_expand_wc of the 1x1 conv's dgrad pack, or Wout_hat itself when the block has no 1x1 conv): h never exists.
 * Writes what edm_conv_out_fwd writes: Fraw (fp32 NCHW, nullable) and D = Fraw * gain_out * c_out + noisy * c_skip.
 * a2 bf16 NHWC [B, H, W, C], cat bf16 NHWC [B, H, W, Cc]; any H, W; deterministic. */
int edm_lowrank_tail_supported(int C, int Cc, int Co, int W);     /* the LDS tables fit (host logic only) */
int edm_lowrank_tail_fwd(const void* a2, const void* cat, const float* Wc, const float* Wp, float sb, float sa,
                         const float* gain_out, const float* noisy, const float* sigma, int sigma_stride, float sigma_data,
                         float* D, float* Fraw, int B, int H, int W, int C, int Cc, int Co, edm_stream_t stream);
/* conv_out's weight gradient without h: gw_hat[o, c] = sb * sum_{t, ci} float(wf2[t][c][ci]) * G[o][t][ci]
 * + sa * sum_cj float(wf1[c][cj]) * G1[o][cj]  (wf1 == NULL: + sa * G1[o][c]); G = edm_lowrank_wgrad(dF, a2, 9),
 * G1 = edm_lowrank_wgrad(dF, cat, 1); wf2 / wf1 = the plain bf16 forward packs [taps][O][I]. */
int edm_lowrank_tail_dwout_supported(int C, int Cc, int Co, int has_1x1);
int edm_lowrank_tail_dwout(const float* G, const void* wf2, const float* G1, const void* wf1, float sb, float sa,
                           float* gw_hat, int Co, int C, int Cc, edm_stream_t stream);
/* d loss / d cat without g_h: bf16(t + sa * dF^T Wp), columns < Ci to gu [B, HW, Ci], the others to gcs [B, HW, Cc - Ci]
 * (gcs == NULL: Ci == Cc); t bf16 NHWC [B, HW, Cc] = the dense part of the gradient. */
int edm_lowrank_gcat_supported(int Cc, int Ci, int Co);
int edm_lowrank_gcat_add(const float* dF, const float* Wp, float sa, const void* t, void* gu, void* gcs, int B, int HW,
                         int Cc, int Ci, int Co, edm_stream_t stream);

int edm_nchw_to_nhwc_bf16(const float* x, void* y, int B, int C, int HW, edm_stream_t stream);
int edm_nhwc_bf16_to_nchw(const void* x, float* y, int B, int C, int HW, edm_stream_t stream);

/* ---------------------------------------------------------------- fp32 linears + embedding (networks.py:58-60, 121-178) */
int edm_linear_fwd(const float* X, const float* W, float* Y, int M, int N, int K, edm_stream_t stream);
/* launch plan of the GEMM C[M,N] (=|+=) A[M,K] B[K,N] the three entry points run (fwd (M,N,K) -> GEMM (M,N,K), dgrad
 * (M,N,K) -> (M,K,N), wgrad (M,N,K) -> (N,K,M)): tile_rows 32 (32x64 tile) or 64 (64x64), splits = K shares added with
 * atomics (C is cleared first when splits > 1 and accumulate == 0).  Host logic only; the launches follow it. */
int edm_linear_plan(int M, int N, int K, int accumulate, int* tile_rows, int* splits);
int edm_linear_dgrad(const float* dY, const float* W, float* dX, int M, int N, int K, int accumulate,
                     edm_stream_t stream);
int edm_linear_wgrad(const float* dY, const float* X, float* dW, int M, int N, int K, int accumulate,
                     edm_stream_t stream);
int edm_fourier_fwd(const float* sigma, int sigma_stride, const float* freqs, const float* phases, float* out, int B,
                    int Fd, edm_stream_t stream);
/* label dropout of classifier-free guidance training (networks.py _EmbeddingFn, Embedding(label_dropout=p)): a dropped
 * sample takes the labels == NULL path for its row.  drop_in (B int32, nullable): the mask, given; otherwise, with
 * drop_out set, drawn per sample b as philox4x32_10((b, 0x4C41424C, 0, step), (seed_lo, seed_hi)).x < drop_thr
 * (drop_thr = round(p * 2^32), at most 2^32; dyn, nullable edm_step_params, overrides step / seed).  drop_out (B int32,
 * nullable) receives the mask used; the backward reads it as drop.  All NULL / 0: the plain combine. */
int edm_embed_combine_fwd(const float* emb_sigma, const float* wcls_hat, const long long* labels, float add_factor,
                          int K, float* pre, float* out, int B, int E, unsigned long long drop_thr,
                          unsigned long long seed, unsigned step, const void* dyn, const int* drop_in, int* drop_out,
                          edm_stream_t stream);
int edm_embed_combine_bwd(const float* gout, const float* pre, const long long* labels, float add_factor, int K,
                          float* gemb_sigma, float* gwcls_hat, int B, int E, const int* drop, edm_stream_t stream);
/* augment-label conditioning (EDM, Karras et al. 2022, App. F.2 -- no reference call site): emb_sigma [B][E] +=
 * aug [B][K] . w_hat [E][K]^T in place (k ascending; an all-zero row changes nothing), before edm_embed_combine_fwd; and
 * gw_hat [E][K] = gemb_sigma^T . aug, summed over b in ascending order (deterministic, no atomics), overwritten. */
int edm_aug_embed_fwd(float* emb_sigma, const float* aug, const float* w_hat, int B, int E, int K, edm_stream_t stream);
int edm_aug_embed_wgrad(const float* gemb_sigma, const float* aug, float* gw_hat, int B, int E, int K,
                        edm_stream_t stream);

/* ---------------------------------------------------------------- step level (edm.py:84-93, 212; metric.py:8-18; edm.py:251; ema.py:137-140; solvers.py:49-57) */
int edm_diffuse(const float* clean, float* noisy, float* sigma, float P_mean, float P_std, int B, long CHW,
                unsigned long long seed, unsigned step, const void* dyn, edm_stream_t stream);
int edm_diffuse_given(const float* clean, const float* eps, const float* noise, float* noisy, float* sigma,
                      float P_mean, float P_std, int B, long CHW, edm_stream_t stream);
/* weight = (sigma^2+sd^2)/(sigma*sd)^2 (edm.py:212) unless weight_override; acc_sum/acc_total (nullable): the metric's
 * epoch state (metric.py:38-49) accumulated in the same pass */
int edm_weighted_mse(const float* D, const float* clean, const float* sigma, const float* weight_override,
                     float sigma_data, float* loss, float* dD, int B, long CHW, float* acc_sum, long long* acc_total,
                     edm_stream_t stream);
/* zero_grad != 0: the gradient arena is cleared in the same pass (optimizer.zero_grad()).
 * health (nullable device word, sticky): bit 0 is OR-ed in when a non-finite gradient / updated weight passed through
 * the step, bit 1 (Heun updates) when the sampler state went non-finite -- the sentinel a replayed hipGraph leaves for
 * the host (Trainer.fit reads it at its log interval, the solver after a solve) so a corrupted replay fails loudly. */
int edm_adam_ema(float* theta, float* grad, float* m, float* v, float* ema, long n, float lr, float b1, float b2,
                 float eps, int step, float ema_beta, float grad_scale, const void* dyn, int zero_grad,
                 unsigned* health, edm_stream_t stream);
/* edm_adam_ema over a set of element ranges of the arenas only; elements outside them are neither read nor written.
 * ranges: DEVICE array of n_ranges (first element, length) pairs of longs; chunks: DEVICE array of n_chunks (range id,
 * offset inside the range) pairs of ints, one per 1024 elements of a range.  Both stay valid and unchanged until the
 * launch has executed (captured stream: for the life of the graph).  n_chunks == 0 launches nothing. */
int edm_adam_ema_ranges(float* theta, float* grad, float* m, float* v, float* ema, long n, const long* ranges,
                        int n_ranges, const int* chunks, int n_chunks, float lr, float b1, float b2, float eps, int step,
                        float ema_beta, float grad_scale, const void* dyn, int zero_grad, unsigned* health,
                        edm_stream_t stream);
/* post-hoc EMA (Karras et al. 2024, Sec. 3): edm_adam_ema plus K = 1..4 profile arenas of n floats, updated from the new
 * weights in the same pass, p_k = beta_k * p_k + (1 - beta_k) * theta_new.  theta / m / v / ema are bitwise those of
 * edm_adam_ema.  profiles: HOST array of K device pointers (16-byte aligned); betas: DEVICE array of K floats read at
 * run time, so a captured step follows the betas the host writes before each replay. */
int edm_adam_ema_phema(float* theta, float* grad, float* m, float* v, float* ema, float* const* profiles, int K,
                       const float* betas, long n, float lr, float b1, float b2, float eps, int step, float ema_beta,
                       float grad_scale, const void* dyn, int zero_grad, unsigned* health, edm_stream_t stream);
/* Guarded optimizer step (grad_guard.hip).  edm_grad_guard reads the gradient arena once and leaves, in DEVICE memory, the
 * per-tensor sums of squares and this 64-byte record; the *_guarded optimizer entry points read the record in the same
 * stream, so a hipGraph-replayed step clips or skips without the host seeing a gradient.
 *   sumsq = sum over tensors of sum (fp32(g) * grad_scale)^2, every square and sum in fp64, in a fixed order (no
 *   floating-point atomics: bit-identical from run to run);  norm = sqrt(sumsq);
 *   coef = min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_; exactly 1 when max_norm is +inf);
 *   skip = skip_nonfinite && (an element is NaN, or |g| or |g * grad_scale| exceeds 3e38).
 * steps / skipped / clipped / consecutive_skips advance when count != 0 (one thread, plain stores). */
typedef struct {
  float coef;
  unsigned skip;
  float norm;
  float clip_value;
  double sumsq;
  unsigned long long steps, skipped, clipped;
  unsigned consecutive_skips;
  unsigned pad[3];
} edm_grad_guard_record;
/* grad: n floats at any 4-byte-aligned address.  chunks: DEVICE table of n_chunks (tensor id, first element, length)
 * triples of longs, no chunk straddling two tensors or covering padding (elements outside the chunks are not read; a chunk
 * that leaves [0, n) is skipped whole); tensors: DEVICE table of n_tensors (first chunk, number of chunks, first block,
 * number of blocks) int quadruples.  The sums are taken over blocks of 1024 elements counted from each tensor's first
 * element (n_blocks in all; every chunk but a tensor's last is a multiple of 1024 long), so the result does not depend on
 * the chunk length.  Both tables stay valid and unchanged until the launches have executed (captured stream: for the life
 * of the graph).  grad_scale / dyn: as edm_adam_ema.  max_norm, clip_value: >= 0, +inf = off.  part (n_blocks doubles) and
 * flags (n_blocks + n_tensors words) are scratch; sumsq (n_tensors doubles) and record (zeroed once by the caller) are the
 * outputs.  Three launches. */
int edm_grad_guard(const float* grad, long n, const long* chunks, int n_chunks, const int* tensors, int n_tensors,
                   int n_blocks, float grad_scale, const void* dyn, float max_norm, float clip_value, int skip_nonfinite,
                   int count, double* part, unsigned* flags, double* sumsq, void* record, edm_stream_t stream);
/* edm_adam_ema / edm_adam_ema_phema behind the guard: the same update expressions with grad_scale * record->coef as the
 * gradient scale and every scaled element limited to +-record->clip_value.  record->skip != 0: theta, m, v, ema and the
 * profiles stay bit for bit, the gradient arena is still cleared when zero_grad != 0, the health word is not touched. */
int edm_adam_ema_guarded(float* theta, float* grad, float* m, float* v, float* ema, long n, float lr, float b1, float b2,
                         float eps, int step, float ema_beta, float grad_scale, const void* dyn, int zero_grad,
                         const void* record, unsigned* health, edm_stream_t stream);
int edm_adam_ema_phema_guarded(float* theta, float* grad, float* m, float* v, float* ema, float* const* profiles, int K,
                               const float* betas, long n, float lr, float b1, float b2, float eps, int step,
                               float ema_beta, float grad_scale, const void* dyn, int zero_grad, const void* record,
                               unsigned* health, edm_stream_t stream);
/* post-hoc EMA reconstruction: acc_l += w_l * snap for l < L <= 8.  acc: device fp64 [L][n], snap: device fp32 [n],
 * w: HOST array of L doubles.  edm_phema_finish rounds n fp64 values to fp32. */
int edm_phema_accumulate(double* acc, const float* snap, const double* w, int L, long n, edm_stream_t stream);
int edm_phema_finish(const double* acc, float* out, long n, edm_stream_t stream);
int edm_heun_euler(const float* x, const float* D, float t0, float t1, float* dx, float* x1, long n, unsigned* health,
                   edm_stream_t stream);
int edm_heun_correct(const float* x, const float* dx, const float* x1, const float* D1, float t0, float t1, float* out,
                     long n, unsigned* health, edm_stream_t stream);
/* guided Heun updates: the two above on D = Dg + w*(Dm - Dg), mixed in registers (no temporary D).  w is a DEVICE
 * pointer to one float, read at run time, so a captured solve follows later writes to it; w == 0 reproduces the
 * unguided update fed Dg bit for bit.  Same health bit. */
int edm_heun_euler_guided(const float* x, const float* Dm, const float* Dg, const float* w, float t0, float t1,
                          float* dx, float* x1, long n, unsigned* health, edm_stream_t stream);
int edm_heun_correct_guided(const float* x, const float* dx, const float* x1, const float* Dm1, const float* Dg1,
                            const float* w, float t0, float t1, float* out, long n, unsigned* health,
                            edm_stream_t stream);
/* churn of the stochastic sampler (Karras et al. 2022, Algorithm 2): x_hat = x + c*n, n ~ N(0, 1) drawn in the kernel,
 * x and x_hat contiguous [B, CHW] fp32.  Element j of sample b is normal j % 4 of one Philox4x32-10 call with counter
 * (j / 4, b, 0x43480000 ^ step, solve_index) and key (seed_lo, seed_hi); the four normals are Box-Muller of words
 * (0, 1) and (2, 3).  rec is a DEVICE pointer to four uint32 {seed_lo, seed_hi, solve_index, 0}, read at run time, so a
 * captured solve draws new noise after the host rewrites it; step and c are by value.  The noise of a sample does not
 * depend on B or on the memory path (dwordx4 when CHW % 4 == 0 and x, x_hat are 16-byte aligned).  Same health bit as
 * the Heun updates. */
int edm_heun_churn(const float* x, float c, const void* rec, int step, int B, long CHW, float* x_hat,
                   unsigned* health, edm_stream_t stream);
/* DPM-Solver++ multistep update (data prediction, sigma(t) = t): m = Dg + w*(Dm - Dg) when guided (Dg and w both
 * non-null; w a DEVICE pointer, as above), else m = Dm; x_out = a*x + c0*m + c1*m1 + c2*m2, with m1 / m2 the
 * previous steps' m (nullable: a null term is absent; m2 needs m1).  m is also written to m_out (nullable), the
 * solver-owned history.  The row (a, c0, c1, c2) = (0, 1, 0, 0) returns m bit for bit.  All operands fp32, n elements,
 * x_out / m_out alias none of them; dwordx4 when every operand is 16-byte aligned.  Same health bit as the Heun
 * updates. */
int edm_dpm_multistep(const float* x, const float* Dm, const float* Dg, const float* w, const float* m1,
                      const float* m2, float a, float c0, float c1, float c2, float* x_out, float* m_out, long n,
                      unsigned* health, edm_stream_t stream);
/* state of an image-conditioned solve at noise level t >= 0: out = image + t*x0 as one fma, x0 the caller's unit
 * noise, all fp32 of n elements.  image is nullable: out = x0*t then, bit for bit what edm_scale_f32 gives.  dwordx4
 * when every operand is 16-byte aligned.  out aliases no operand.  Same health bit as the Heun updates. */
int edm_state_init(const float* image, const float* x0, float t, float* out, long n, unsigned* health,
                   edm_stream_t stream);
/* replacement step of inpainting (Song et al. 2021): out = mask ? image + t*n : x, n ~ N(0, 1) drawn in the kernel,
 * x / image / out contiguous [B, C, HW] fp32, t >= 0.  mask: uint8 [mask_B, HW], mask_B in {1, B}, broadcast over the
 * channels (and the batch when mask_B == 1); non-zero = known pixel, taken from image.  Element j of sample b (j over
 * C*HW) is normal j % 4 of one Philox4x32-10 call with counter (j / 4, b, 0x49500000 ^ step, solve_index) and key
 * (seed_lo, seed_hi), Box-Muller of words (0, 1) and (2, 3) as edm_heun_churn; the tag differs from the churn's
 * 0x43480000 (and from edm_diffuse's 0xD1FF / 0x5167), so the two streams of one (seed, solve_index, step) are
 * independent; step < 65536.  rec is the churn's DEVICE record {seed_lo, seed_hi, solve_index, 0}, read at run time.
 * The noise of a sample does not depend on B, the mask or the memory path (dwordx4 and one 32-bit mask load per quad when
 * HW % 4 == 0, x / image / out are 16-byte and mask 4-byte aligned).  t == 0 returns image bit for bit on the mask.
 * Same health bit as the Heun updates. */
int edm_inpaint_blend(const float* x, const float* image, const unsigned char* mask, float t, const void* rec, int step,
                      int B, int C, long HW, int mask_B, float* out, unsigned* health, edm_stream_t stream);
/* zero-shot restoration from a linear measurement y = A x (DDNM, Wang et al. 2023; restore.hip).  A averages every
 * scale x scale pixel block, scale in {1, 2, 4, 8} with H % scale == 0 and W % scale == 0, and with gray != 0 also the
 * C <= 8 channels; its pseudo-inverse A+ replicates a value to its block (A A+ = I, A+ A an orthogonal projector).
 * scale == 1 without gray is the identity and is refused.  x / Dm / Dg / out: contiguous [B, C, H, W] fp32; y:
 * contiguous [B, gray ? 1 : C, H/scale, W/scale] fp32.
 * edm_degrade: y = A x.
 * edm_project_denoised: D = Dg + w*(Dm - Dg) when Dg and w are both non-null (w a DEVICE pointer to one float, read at
 *   run time as in edm_heun_euler_guided, so a captured solve follows later writes to it; w == 0 equals the unguided
 *   call fed Dg bit for bit), else D = Dm;  out = D + (y_block - mean_block(D)): the projection of D onto {x : A x = y}.
 *   out aliases no operand.  Same health bit as the Heun updates when an element of out is non-finite.
 * The block mean is the same code in both and order-fixed (no atomics, no cross-thread reduction: one thread owns whole
 * blocks): acc = 0, then acc += D[c][row][column] in sequential fp32 adds with the channels ascending (gray only), then
 * the rows of the block, then its columns; mean = acc * (1.0f / n), n = scale*scale*(gray ? C : 1), one multiplication.
 * The correction is one subtraction y - mean per block and one addition per element, none contracted with another
 * operation.  Hence project(D, degrade(D)) == D and project(0, y) == A+ y bit for bit, and a sample's result depends
 * neither on B nor on the memory path: with W % 4 == 0 and every fp32 operand 16-byte aligned a thread reads its rows
 * as dwordx4 (two blocks of a row for scale 2, one for 4, two loads for 8; neighbouring threads take neighbouring strips
 * of the same rows), otherwise one block per thread element by element, with the same bits. */
int edm_degrade(const float* x, float* y, int B, int C, int H, int W, int scale, int gray, edm_stream_t stream);
int edm_project_denoised(const float* Dm, const float* Dg, const float* w, const float* y, float* out, int B, int C,
                         int H, int W, int scale, int gray, unsigned* health, edm_stream_t stream);
/* Diffusion posterior sampling (Chung et al. 2023; restore.hip): the measurement side of a step x' + (zeta / ||r||) g with
 * r = y - A D and g = J^T A^T r.  All tensors contiguous fp32; no output aliases an operand.
 * edm_degrade_adjoint: out [B, C, H, W] = A^T r for the averaging A of edm_degrade (r of the measurement shape): every value
 *   replicated to its block (and, gray, to the C channels) times 1.0f / n, n = scale*scale*(gray ? C : 1).
 * edm_blur2d: y = K x on each of `planes` H x W planes, K the separable blur with the 2*radius+1 taps `taps` (a HOST
 *   pointer, copied into the launch; radius 1..4) and ZERO padding -- with symmetric taps K is its own adjoint.  Both passes
 *   are fma chains over all taps in ascending order (a tap off the map adds 0).
 * edm_dps_residual: r = y - AD over [B, n] and nrm[b] = sqrt(sum_i r[b,i]^2): thread t of the sample's workgroup adds the
 *   squares of elements t, t + 256, ... in that order, then a fixed binary tree over the 256 partial sums -- no atomics:
 *   the same bits on every run, whatever B.
 * edm_dps_update: out[b,:] = x[b,:] + (scale / nrm[b]) * g[b,:] (one division per sample, one fma per element); out = x bit
 *   for bit where nrm[b] == 0 or scale == 0.  Same health bit as the Heun updates. */
int edm_degrade_adjoint(const float* r, float* out, int B, int C, int H, int W, int scale, int gray, edm_stream_t stream);
int edm_blur2d(const float* x, float* y, const float* taps, int radius, long planes, int H, int W, edm_stream_t stream);
int edm_dps_residual(const float* y, const float* AD, float* r, float* nrm, int B, long n, edm_stream_t stream);
int edm_dps_update(const float* x, const float* g, const float* nrm, float scale, float* out, int B, long n,
                   unsigned* health, edm_stream_t stream);
/* Likelihood evaluation along the probability-flow ODE dx/dt = (x - D(x; t)) / t: the Heun updates plus the integral of
 * the drift's divergence (CHW - tr dD/dx) / t, the trace estimated without a backward pass (Hutchinson with Rademacher
 * probes, central difference through the network):
 *   q_b = 1/K sum_p sum_j eps_pj (D(x + h eps_p)_bj - D(x - h eps_p)_bj) / (2h).
 * An evaluation batch is [(1 + 2K) B, CHW] fp32: rows [0, B) the state x, rows [(1 + 2p) B, (2 + 2p) B) x + h eps_p,
 * rows [(2 + 2p) B, (3 + 2p) B) x - h eps_p (one fp32 add each), 1 <= K <= 32.  eps is never stored: element j of sample
 * b (j over CHW) takes bit p of word j % 4 of one Philox4x32-10 call with counter
 * (j / 4, b, (0x4E4C0000 + (ev << 16)) ^ step, solve_index) and key (seed_lo, seed_hi); bit clear = +1, set = -1; ev = 0
 * for the Euler evaluation of step `step`, 1 for its correction; step < 65536, so the tags differ from the churn's
 * 0x43480000 and the blend's 0x49500000 whatever the steps are.  rec is the churn's DEVICE record {seed_lo, seed_hi,
 * solve_index, 0}, read at run time.  The bits do not depend on B or on the memory path (dwordx4 when CHW % 4 == 0 and
 * every fp32 operand is 16-byte aligned, else element by element).  Outputs alias no operand.
 * Reductions are order-fixed (no floating-point atomics): per-(sample, chunk) fp64 partials go to `part`, a DEVICE
 * workspace of B * EDM_NLL_MAX_CHUNKS doubles, and a one-thread-per-sample finish launch adds them in index order into
 * L, DEVICE fp64 [B], += in place.  Same health bit as the Heun updates (also set when L goes non-finite).
 *
 * edm_nll_probe: E = the evaluation batch of x [B, CHW] with half-width h under (step, ev).
 * edm_heun_euler_div: edm_heun_euler on rows [0, B) of (E, D): dx [B, CHW], and E1 = the evaluation batch of x1 with
 *   half-width h1 under (step, 1);  L_b += (t1 - t0) / 2 * (CHW - q_b) / t0 with q_b from D under (step, 0) and h0.
 * edm_heun_correct_div: edm_heun_correct on rows [0, B) of (E, dx, E1, D1): out = the evaluation batch of the new state
 *   with half-width hn under (step - 1, 0) (the next step's Euler evaluation) when probes_out != 0, else the new state
 *   alone, [B, CHW];  L_b += (t1 - t0) / 2 * (CHW - q_b) / t1 with q_b from D1 under (step, 1) and h1.
 * edm_nll_prior: L_b += log N(x_b; 0, t^2 I) = -CHW/2 log(2 pi t^2) - sum_j (x_bj / t)^2 / 2, x [B, CHW]. */
#define EDM_NLL_MAX_CHUNKS 64
/* How many entries of a sample's row of `part` the order-fixed reductions fill (likelihood, noise-level evaluation, the
 * adaptive and the parallel solver): min(ceil(ceil(CHW / 4) / 256), EDM_NLL_MAX_CHUNKS), 0 for CHW <= 0.  Host logic only:
 * the rule the kernels index with, asked of the library instead of restated by the caller. */
int edm_sample_chunks(long CHW);
int edm_nll_probe(const float* x, float h, const void* rec, int step, int ev, int K, int B, long CHW, float* E,
                  unsigned* health, edm_stream_t stream);
int edm_heun_euler_div(const float* E, const float* D, float t0, float t1, float h0, float h1, const void* rec, int step,
                       int K, int B, long CHW, float* dx, float* E1, double* part, double* L, unsigned* health,
                       edm_stream_t stream);
int edm_heun_correct_div(const float* E, const float* dx, const float* E1, const float* D1, float t0, float t1, float h1,
                         float hn, const void* rec, int step, int K, int probes_out, int B, long CHW, float* out,
                         double* part, double* L, unsigned* health, edm_stream_t stream);
int edm_nll_prior(const float* x, float t, int B, long CHW, double* part, double* L, unsigned* health,
                  edm_stream_t stream);
/* Loss by noise level (tinyedm_amd/evaluate.py): the denoising error of held-out images at fixed noise levels with fixed
 * noise, a number that is the same for the same checkpoint on every run.
 * edm_eval_diffuse: noisy_b = clean_b + sigma_b * n as one fma per element, sigma_b = sigmas[level[b]], and
 *   sigma_out[b] = sigma_b.  clean / noisy: contiguous [B, CHW] fp32; ids: DEVICE uint32 [B], the image's index in the
 *   evaluation set; level: DEVICE int32 [B] with 0 <= level[b] < L; sigmas: DEVICE float [L], 1 <= L <= 65535; sigma_out:
 *   DEVICE float [B].  n ~ N(0, 1) is drawn in the kernel and belongs to the image, not to the row: element j of sample b
 *   is normal j % 4 of one Philox4x32-10 call with counter (j / 4, ids[b], 0x45560000 ^ level[b], draw) and key
 *   (seed_lo, seed_hi), Box-Muller of words (0, 1) and (2, 3) as edm_heun_churn.  level < 65536, so the tag differs from
 *   the churn's 0x43480000, the blend's 0x49500000, the probes' 0x4E4C0000 + (ev << 16) and edm_diffuse's 0xD1FF / 0x5167.
 *   rec is the churn's DEVICE record {seed_lo, seed_hi, draw, 0}, read at run time.  The noise of an (id, level, draw)
 *   does not depend on B, on the row, on the other rows or on the memory path (dwordx4 when CHW % 4 == 0 and clean, noisy
 *   are 16-byte aligned, else element by element with the same bits).  The caller validates level; the kernel uses no
 *   unchecked value as an index: a level outside [0, L) gives that row sigma = NaN and sets the health bit.  Same health
 *   bit as the Heun updates when an output is non-finite.
 * edm_eval_sqerr: se[b] = sum_j ((double)D_bj - (double)clean_bj)^2, D / clean contiguous [B, CHW] fp32, B <= 65535; se
 *   is a DEVICE fp64 [B] slice, WRITTEN (it may point into a larger result matrix).  Order-fixed, no floating-point
 *   atomics: per-(sample, chunk) fp64 partials go to `part`, a DEVICE workspace of B * EDM_NLL_MAX_CHUNKS doubles, and a
 *   one-thread-per-sample finish launch adds them in index order.  A sample's chunking depends on CHW alone, so se[b] is
 *   bit-identical whatever B, the row or the memory path (dwordx4 when CHW % 4 == 0 and D, clean are 16-byte aligned).
 *   Same health bit when se[b] is non-finite.
 * The class sweep (tinyedm_amd/classify.py): one network call holds P (image, level) pairs x C classes, row p * C + c is
 * pair p under class c (the class index fastest).  Both are the kernels above with a row divisor C; C = 1 is the pair above.
 * edm_eval_diffuse_classes: clean [P, CHW], ids / level DEVICE [P]; noisy [P * C, CHW] and sigma_out [P * C].  The noise
 *   of a pair is drawn once per element and stored to its C rows: row p * C + c of noisy and sigma_out holds exactly the
 *   bits edm_eval_diffuse writes for pair p, so the classes of an (image, level, draw) meet the same noise.  P * C < 2^31.
 *   Level checking, health bit and memory paths as edm_eval_diffuse (dwordx4 when CHW % 4 == 0 and clean, noisy are
 *   16-byte aligned: every row then is).
 * edm_eval_sqerr_classes: se[p * C + c] = sum_j ((double)D_(p*C+c)j - (double)clean_pj)^2 with the bits edm_eval_sqerr
 *   gives for row D[p * C + c] against clean[p] (chunking, thread-to-quad assignment, block reduction and finish order
 *   are the same code); D contiguous [P * C, CHW], clean contiguous [P, CHW] and never replicated in memory,
 *   P * C <= 65535; part: DEVICE workspace of P * C * EDM_NLL_MAX_CHUNKS doubles; se: DEVICE fp64 [P * C] slice, WRITTEN. */
int edm_eval_diffuse(const float* clean, const unsigned* ids, const int* level, const float* sigmas, int L,
                     const void* rec, int B, long CHW, float* noisy, float* sigma_out, unsigned* health,
                     edm_stream_t stream);
int edm_eval_sqerr(const float* D, const float* clean, int B, long CHW, double* part, double* se, unsigned* health,
                   edm_stream_t stream);
int edm_eval_diffuse_classes(const float* clean, const unsigned* ids, const int* level, const float* sigmas, int L,
                             const void* rec, int P, int C, long CHW, float* noisy, float* sigma_out, unsigned* health,
                             edm_stream_t stream);
int edm_eval_sqerr_classes(const float* D, const float* clean, int P, int C, long CHW, double* part, double* se,
                           unsigned* health, edm_stream_t stream);
int edm_scale_f32(const float* x, float s, float* y, long n, edm_stream_t stream);

/* ---------------------------------------------------------------- adaptive ODE solver (adaptive.hip)
 * The embedded Heun(2) / Euler(1) pair with local extrapolation, every sample at its own time and step size; the hot
 * path reads nothing on the host.  x, D, dx, x1, y are contiguous fp32 [B, CHW].
 * state: DEVICE, EDM_ADAPT_ROWS rows of B 32-bit words, row r at (uint32*)state + r * B:
 *   0 t (fp32, the current time), 1 t1 (fp32, the trial time), 2 h (fp32, signed, the next proposal), 3 err (fp32, the
 *   last E), 4 status (uint32: 0 active, 1 done, 2 failed), 5 accepted, 6 rejected (uint32 counters), 7 after_reject
 *   (uint32: the last controlled step was a rejection).
 * Snap rule: the trial time of a step h from t is t + h (fp64 sum, rounded to fp32), but t_end exactly when t + h passes
 *   t_end or comes within 0.01 |h| of it.  A sample that is not active has t1 == t.
 * edm_adapt_begin: t = t_start, h = h0 (non-zero, pointing from t_start to t_end; both times > 0), status = active,
 *   counters and err zero, t1 by the snap rule.
 * edm_adapt_euler: edm_heun_euler with t0 = t[b], t1 = t1[b] (DEVICE fp32 [B]) read per sample: with every sample at one
 *   pair (t0, t1) it gives edm_heun_euler's bits.  A sample with t1[b] == t[b] gets x1 = x, dx = 0 whatever D holds.
 *   dwordx4 when CHW % 4 == 0 and x, D, dx, x1 are 16-byte aligned, the same bits element by element otherwise.  Same
 *   health bit as the Heun updates.
 * edm_adapt_correct: y = x + (t1 - t0)(dx/2 + ((x1 - D1)/t1)/2) with edm_heun_correct's bits under the same condition
 *   (y = x where t1[b] == t[b]), and part[b][chunk] = the chunk's share of
 *   sum_j ((y_j - x1_j) / (atol + rtol max(|x_j|, |y_j|)))^2, every term in fp64 from the fp32 values.  part: DEVICE
 *   workspace of B * EDM_NLL_MAX_CHUNKS doubles; the chunking depends on CHW alone and there are no floating-point
 *   atomics, so a sample's sum has the same bits whatever B, its row, its neighbours or the memory path (the rule of
 *   edm_eval_sqerr).  B <= 65535; atol, rtol >= 0, not both 0.  Same health bit.
 * edm_adapt_control: one thread per ACTIVE sample, fp64: E = sqrt(sum_chunks part[b][.] / CHW) in index order; accept iff
 *   E <= 1 (a NaN E rejects); factor = clamp(safety / sqrt(E), fac_min, top), top = fac_max, or 1 on a rejection and on
 *   the step after one (a NaN factor is fac_min); h = (t1 - t) * factor; on accept t = t1, accepted++, status = done when
 *   t == t_end; otherwise rejected++.  A sample still active with |h| < h_floor |t| becomes failed and sets the health
 *   bit of the Heun updates.  Then t1 by the snap rule (t1 = t unless active).  accept: DEVICE uint8 [B], WRITTEN for
 *   every sample (0 for one that was not active); active: DEVICE int32, += the number of samples still active.
 *   0 < safety <= 1, 0 < fac_min < 1 <= fac_max < inf, 0 <= h_floor < 1.
 * edm_adapt_commit: x = accept[b] ? y : x in place; a sample with accept[b] == 0 is not written.  dwordx4 when
 *   CHW % 4 == 0 and x, y are 16-byte aligned. */
#define EDM_ADAPT_ROWS 8
int edm_adapt_begin(float t_start, float t_end, float h0, int B, void* state, edm_stream_t stream);
int edm_adapt_euler(const float* x, const float* D, const float* t, const float* t1, int B, long CHW, float* dx,
                    float* x1, unsigned* health, edm_stream_t stream);
int edm_adapt_correct(const float* x, const float* dx, const float* x1, const float* D1, const float* t, const float* t1,
                      int B, long CHW, double atol, double rtol, float* y, double* part, unsigned* health,
                      edm_stream_t stream);
int edm_adapt_control(const double* part, int B, long CHW, float t_end, double safety, double fac_min, double fac_max,
                      double h_floor, void* state, unsigned char* accept, int* active, unsigned* health,
                      edm_stream_t stream);
int edm_adapt_commit(float* x, const float* y, const unsigned char* accept, int B, long CHW, edm_stream_t stream);

/* ---------------------------------------------------------------- parallel-in-time sampling (picard.hip)
 * Picard iteration of the Heun / Euler step over a window of P <= EDM_PICARD_MAX_WINDOW consecutive steps of a sigma
 * table t_0 .. t_{N-1} (N >= 2), every sample with its own window start s_b; the hot path reads nothing on the host.
 * Window position j = 0 .. P of sample b stands at table index s_b + j: position 0 is converged, the next
 * L_b = min(P, N - 1 - s_b) are live, the rest are inactive.  Position-major buffers: X, Xnew fp32 [P + 1][B][CHW]; dx,
 * X1, D, D1 fp32 [P][B][CHW] (row j: the Euler stage / network outputs of position j); T fp32 [P + 1][B],
 * T[j][b] = t[min(s_b + j, N - 1)].
 * state: DEVICE, EDM_PICARD_ROWS rows of B 32-bit words: 0 start (s_b), 1 status (0 active, 1 done), 2 iterations.
 * edm_picard_scan: new_0 = X[0]; new_{j+1} = fma(t1 - t0, 0.5 dx_j + 0.5 (X1_j - D1_j) / t1, new_j) (D1 == NULL: the
 *   Euler iteration fma(t1 - t0, dx_j, new_j)) for the live j, with edm_heun_correct's / edm_heun_euler's bits where
 *   new_j == X[j]; inactive positions copy new_L and nothing of theirs but X is read.  part[b][j][chunk] (DEVICE doubles
 *   [B][P][chunks], chunks = min(ceil(ceil(CHW / 4) / 256), EDM_NLL_MAX_CHUNKS)) = the chunk's share of
 *   sum ((new - old) / (atol + rtol max(|old|, |new|)))^2 over position j + 1, fp64, order-fixed as edm_adapt_correct's (a
 *   zero scale contributes 0 where new == old and +inf otherwise); 0 for an inactive position.  tol: DEVICE doubles
 *   {atol, rtol}, both >= 0 (both 0: converged = unchanged bit for bit).  Health bit of the Heun updates on a non-finite
 *   live state.  dwordx4 when CHW % 4 == 0 and the buffers are 16-byte aligned, the same bits otherwise.  B <= 65535.
 * edm_picard_control: one thread per ACTIVE sample, fp64: E_j = sqrt(sum_chunks part[b][j-1][.] / CHW) in index order for
 *   j = 1 .. L_b (written to err[b][j-1] when err != NULL); m = the leading positions with E_j <= 1 (NaN: not converged);
 *   stride[b] = min(m + 1, L_b) (0 for a sample that was not active); s_b += stride, iterations++, done when
 *   s_b == N - 1.  active: DEVICE int32, += the number of samples still active.
 * edm_picard_slide: X[j] = Xnew[j + r] while j + r <= L (r = stride[b], L the live length before the slide, the state
 *   already advanced); a position entering at table index i <= N - 1 gets fma(Xnew[L] - Dh, t_i / t_{s+L}, Dh) with
 *   Dh = D[L-1]; indices past N - 1 copy Xnew[L]; T is rewritten.  X must not alias Xnew.  begin != 0: Xnew is the unit
 *   noise [B][CHW]; X[j] = t_j * Xnew (copies of X[0] past N - 1), T and the state (s = 0, active, 0 iterations) are
 *   written; D and stride are not read.  t_table: DEVICE fp32, >= N entries. */
#define EDM_PICARD_ROWS 3
#define EDM_PICARD_MAX_WINDOW 64
int edm_picard_scan(const float* X, const float* dx, const float* X1, const float* D1, const float* T, const void* state,
                    const double* tol, int B, int N, int P, long CHW, float* Xnew, double* part, unsigned* health,
                    edm_stream_t stream);
int edm_picard_control(const double* part, int B, long CHW, int N, int P, void* state, int* stride, double* err,
                       int* active, edm_stream_t stream);
int edm_picard_slide(const float* Xnew, const float* D, const int* stride, void* state, const float* t_table, int begin,
                     int B, int N, int P, long CHW, float* X, float* T, edm_stream_t stream);

/* ---------------------------------------------------------------- reference-precision evaluation (eval_f32.hip)
 * The reference samples / validates in fp32 (generate.py:39-44, callbacks.py:41-49, solvers.py:43-59).  These entry
 * points are the exact-fp32 forward: NHWC fp32 activations [pixels][channels], fp32 effective weights (the w_hat arrays
 * of edm_weight_prep: [Cout][I*taps], master OIHW order), every convolution on v_mfma_f32_32x32x2_f32 (fp32 products,
 * fp32 sums).  Forward only, eval semantics (no dropout, no in-place weight normalisation). */
/* Y = alpha*conv(X, w_hat) + beta*R, or (lin != NULL) the block's modulation epilogue Y = mp_silu(alpha*conv *
 * (lin[b,:]*gain + 1)) (networks.py:253-260).  taps in {1,9}; Cin % 8 (3x3) / % 32 (1x1); I <= Cin (X zero-padded). */
int edm_f32_conv(const float* X, const float* w_hat, float* Y, const float* R, float alpha, float beta, const float* lin,
                 long lin_stride, const float* gain, int B, int H, int W, int Cin, int I, int Cout, int taps,
                 edm_stream_t stream);
/* Split-bf16 form of the same evaluation (round 4): an fp32-accurate convolution at a third of the bf16 kernels' rate
 * instead of the f32-MFMA rate (1/16).  An fp32 value travels as a PAIR of bf16, hi = bf16(x), lo = bf16(x - hi):
 * edm_f32_to_pairs turns [rows][C] floats into [rows][2 C] bf16 = [hi | lo]; edm_split_pack turns w_hat [O][I*taps] into
 * [taps][O][3 Ip] bf16 = [w_hi | w_lo | w_hi]; edm_split_conv accumulates hi.w_hi + hi.w_lo + lo.w_hi in fp32 (what is
 * dropped, lo.w_lo, is 2^-18 of a product) and writes FLOATS: Y = alpha*conv + beta*R (R floats), or, with lin,
 * Y = mp_silu(conv * (lin[b,:]*gain + 1)); Ypairs (optional; Y may then be NULL) receives the same result as pairs, the
 * next conv's Xp.  C % 32 == 0, Cout % 8 == 0, taps in {1, 9}. */
int edm_f32_to_pairs(const float* x, void* pairs, long rows, int C, edm_stream_t stream);
int edm_split_pack(const float* w_hat, void* pack, int O, int I, int taps, int Ip, edm_stream_t stream);
int edm_split_conv(const void* Xp, const void* Wp3, float* Y, void* Ypairs, const float* R, float alpha, float beta,
                   const float* lin, long lin_stride, const float* gain, int B, int H, int W, int C, int Cout, int taps,
                   edm_stream_t stream);
/* the same with an output descriptor for the pairs (round 6; how the split evaluation's torch.cat((input, skip * gate)),
 * networks.py:311, stops being a copy): Ypairs rows have ld_pairs elements (0 = 2 Cout) and the lo halves sit lo_off elements
 * behind the hi halves (0 = Cout) -- i.e. Ypairs may be the left column blocks of the NEXT decoder block's concatenated
 * operand [hi(Ci + Cs) | lo(Ci + Cs)]; Ysilu_pairs (optional) receives mp_silu of the result as pairs at the same offsets of
 * a second buffer (that block's first 3x3 conv reads it, networks.py:316).  Any of Y / Ypairs / Ysilu_pairs may be NULL
 * (not all three).  edm_f32_skip_half fills the right column blocks (the gated skip and mp_silu of it). */
int edm_split_conv_o(const void* Xp, const void* Wp3, float* Y, void* Ypairs, long ld_pairs, long lo_off, void* Ysilu_pairs,
                     const float* R, float alpha, float beta, const float* lin, long lin_stride, const float* gain, int B,
                     int H, int W, int C, int Cout, int taps, edm_stream_t stream);
/* edm_conv3x3_fold for the split evaluation: Y = alpha3 * conv3x3(Xp, Wp3) + alpha1 * conv1x1(X2p, W2p3); X2p [pixels][2 C2]
 * pairs, W2p3 [Cout][3 C2]; outputs as edm_split_conv_o; -3 where the folded form is not built (the caller keeps two launches) */
int edm_split_conv_fold(const void* Xp, const void* Wp3, const void* X2p, const void* W2p3, int C2, float* Y, void* Ypairs,
                        long ld_pairs, long lo_off, void* Ysilu_pairs, float alpha3, float alpha1, int B, int H, int W, int C,
                        int Cout, edm_stream_t stream);
int edm_f32_skip_half(const float* skip, const float* gate, void* cat_pairs, void* silu_pairs, int B, int HW, int Ci, int Cs,
                      edm_stream_t stream);
/* cosine attention (networks.py:194-202) on the qkv conv's own output order: channel head*3d + 3*dd + {q,k,v};
 * y [B*N][C] with channel head*d + dd.  head_dim in {32, 64, 128, 144, 192}; any number of tokens (key tiles of 64). */
int edm_f32_attention(const float* qkv, float* y, int B, int N, int C, int heads, edm_stream_t stream);
/* the same attention for the split-bf16 ("f32x3") evaluation path: every matrix product in three bf16 MFMA passes over
 * (hi, lo) operand pairs (fp32-accurate to 2^-17 per operand, as edm_split_conv), normalisation / softmax / accumulation in
 * fp32.  y (fp32 [B*N][C]) and / or ypairs (bf16 [B*N][2C] = [hi | lo], the out conv's operand format) -- either may be
 * NULL.  head_dim 64 and N <= 256 tokens; -3 otherwise (callers fall back to edm_f32_attention). */
int edm_split_attention(const float* qkv, float* y, void* ypairs, int B, int N, int C, int heads, edm_stream_t stream);
/* (s_pairs / pairs_row / pairs != 0 in the three entry points below: the mp_silu / concat outputs are written as split-bf16
 * PAIRS -- rows [hi(C) | lo(C)] of bf16 in the same bytes -- ready to be edm_split_conv's Xp) */
int edm_f32_pixelnorm_silu(const float* x, float* xn, float* s, long P, int C, int s_pairs, edm_stream_t stream);
int edm_f32_silu(const float* x, float* s, long n, int pairs_row, edm_stream_t stream);
int edm_f32_pool2(const float* x, float* y, int B, int Hout, int Wout, int C, edm_stream_t stream);
int edm_f32_up2(const float* x, float* y, int B, int Hout, int Wout, int C, edm_stream_t stream);
/* round 6, one pass each: EncD blocks without a 1x1 conv (networks.py:246-252): 2x2 average pool -> pixel norm -> mp_silu,
 * the pooled tensor never written (bit-identical to edm_f32_pool2 + edm_f32_pixelnorm_silu; C <= 1024); DecU blocks
 * (networks.py:312-316): y = nearest-exact x2 of x and s = mp_silu(y) (floats, or pairs when s_pairs != 0) */
int edm_f32_pool_pixelnorm_silu(const float* x, float* xn, float* s, int B, int Hout, int Wout, int C, int s_pairs,
                                edm_stream_t stream);
int edm_f32_up2_silu(const float* x, float* y, float* s, int B, int Hout, int Wout, int C, int s_pairs, edm_stream_t stream);
/* ScaleLong gate of a skip tensor (networks.py:112-118): mean over H*W in a fixed order + the gate MLP, per sample */
int edm_f32_skip_gate(const float* skip, const float* W1h, const float* W2h, float* gate, int B, int HW, int C, int R,
                      edm_stream_t stream);
int edm_f32_concat_gate(const float* inp, const float* skip, const float* gate, float* cat, float* silu_out, int B,
                        int HW, int Ci, int Cs, int pairs, edm_stream_t stream);
int edm_f32_precond_in(const float* noisy, const float* sigma, int sigma_stride, float sigma_data, float* out, int B,
                       int Cimg, int HW, int CP, edm_stream_t stream);
int edm_f32_conv_out(const float* x, const float* w_hat, const float* gain_out, const float* noisy, const float* sigma,
                     int sigma_stride, float sigma_data, float* D, int B, int HW, int C, int Co, edm_stream_t stream);
int edm_f32_nchw_to_nhwc(const float* x, float* y, int B, int C, int HW, edm_stream_t stream);
int edm_f32_nhwc_to_nchw(const float* x, float* y, int B, int C, int HW, edm_stream_t stream);

/* ---------------------------------------------------------------- data formats either side of the path */
/* resident uint8 dataset [N][C][H][W] -> fp32 NCHW batch: sample b = image index[b]; (x/255 - mean)/std with the
 * optional per-sample horizontal flip (datamodules/cifar10datamodule.py:18-32, mnistdatamodule.py:18-30). */
int edm_u8_gather_normalize(const void* data, const long* index, float* out, int B, int C, int H, int W, long n_images,
                            float mean, float stdv, int flip, unsigned long long seed, unsigned epoch,
                            edm_stream_t stream);
/* edm_u8_gather_normalize with the non-leaking augmentation of EDM composed into the gather (Karras et al. 2022,
 * "Elucidating the Design Space of Diffusion-Based Generative Models", App. F.2 -- the reference has no call site): the
 * exact, pixel-permuting subset xflip, yflip, whole-pixel translation (border reflected without edge repeat), rot90.
 * Each op of aug_ops (bit 0 xflip, 1 yflip, 2 translate, 3 rot90) is enabled per sample iff its Philox word < aug_thr
 * (round(p * 2^32), at most 2^32); `flip` keeps its meaning and is applied first.  aug [B][6] fp32 receives the augment
 * labels (xflip, yflip, sx / W, sy / H, cos(k pi/2) - 1, sin(k pi/2)); zeros for a disabled op.  rot90 with H != W:
 * status -3 (unsupported), nothing is launched.  The word -> draw mapping is written down at aug_draw in csrc/data.hip. */
int edm_u8_gather_augment_normalize(const void* data, const long* index, float* out, int B, int C, int H, int W,
                                    long n_images, float mean, float stdv, int flip, unsigned long long seed,
                                    unsigned epoch, unsigned long long aug_thr, int aug_ops, float* aug,
                                    edm_stream_t stream);
/* edm_u8_gather_augment_normalize followed by the continuous ops of the same pipe: zoom, rotate, stretch, shift (the
 * project's own definition: 2x upsampling with the sym6 low-pass taps over a reflected border, a bilinear warp on the 2x
 * grid, 2x downsampling with the same taps; DESIGN.md, "Continuous augmentation"; draws and labels at
 * k_u8_gather_warp_normalize in csrc/data.hip).  warp_ops: bit 0 zoom, 1 rotate, 2 stretch, 3 shift, enabled per sample
 * like the exact ops.  aug [B][13] fp32: the six labels above, then (n_s, cos(theta) - 1, sin(theta), n_a cos(phi),
 * n_a sin(phi), n_x, n_y).  theta [B][6] fp32 (may be null) receives each sample's 2x3 matrix on the 2x grid.  A sample with
 * no continuous op enabled is edm_u8_gather_augment_normalize's bit for bit.  H or W outside 2 .. 64, or rot90 with
 * H != W: status -3 (unsupported), nothing is launched.  An out-of-range index entry skips that sample's rows. */
int edm_u8_gather_augment_warp_normalize(const void* data, const long* index, float* out, int B, int C, int H, int W,
                                         long n_images, float mean, float stdv, int flip, unsigned long long seed,
                                         unsigned epoch, unsigned long long aug_thr, int aug_ops, int warp_ops,
                                         float* aug, float* theta, edm_stream_t stream);
/* (x*scale + offset).clip(0,255) -> uint8, layout preserved (cifar10datamodule.py:34-35: scale 127.5, offset 128) */
int edm_denormalize_u8(const float* x, void* out, long n, float scale, float offset, edm_stream_t stream);
/* clamp(pred*std[c]*2 + mean[c], 0, 1)*255 -> uint8 NHWC (callbacks.py:126-156, PreditionWriter) */
int edm_prediction_to_u8_nhwc(const float* pred, void* out, int B, int C, int H, int W, const float* mean,
                              const float* stdv, edm_stream_t stream);

/* ---------------------------------------------------------------- exact nearest neighbours of uint8 images (csrc/neighbors.hip) */
/* For every query row the k reference rows with the smallest key (d2, reference index), d2 = sum_j (q_j - r_j)^2 as an exact
 * integer (int8 MFMA on the rows shifted by 128, int32 accumulation); ties in distance go to the lower index, so the result
 * is unique and independent of tiling, split count and chunking.  Limits, status -1 otherwise: 1 <= D <= 32768 (then
 * 65025 D < 2^31), 1 <= k <= 32, k <= R (k <= R - 1 with exclude_self), R <= 2^31 - 128.
 * edm_u8_knn_splits: the number of shares of the R axis the library would give a Q x R search (host logic only).
 * edm_u8_norms: norms[row] = sum_j (x_j - 128)^2 of x u8 [n_rows][D], the row norms edm_u8_knn_partial takes; once per set.
 * edm_u8_knn_partial: queries u8 [Q][D], refs u8 [R][D], row-contiguous at any byte alignment (16-byte loads when both bases
 *   are 16-byte aligned and D % 16 == 0, element loads otherwise; same results), qnorms [Q] and rnorms [R] their
 *   edm_u8_norms.  Writes keys [splits][Q][k]: uint64 d2 << 32 | (ref_base + reference row), each list ascending, unused
 *   slots all-ones.  `splits` is the caller's choice in [1, 1024].  exclude_self skips the reference whose reported index
 *   equals the query row.  partial != 0 waives k <= R for a chunk of a larger reference set that the caller has checked as
 *   a whole.  Further limits: Q <= 65535 * 128, ref_base + R <= 2^31 - 128 (row numbers of the last tile stay ints).
 * edm_knn_merge: keys [n_lists][Q][k] (the splits of one call, or of every chunk of a chunked search, end to end) ->
 *   dist uint32 [Q][k], idx int32 [Q][k], ascending by key.  Each query needs k non-empty keys across its lists.  No atomics
 *   anywhere; every output element is written by ordinary stores. */
int edm_u8_knn_splits(long Q, long R);
int edm_u8_norms(const void* x, long n_rows, int D, int* norms, edm_stream_t stream);
int edm_u8_knn_partial(const void* queries, const void* refs, long Q, long R, int D, int k, int exclude_self, long ref_base,
                       int partial, int splits, const int* qnorms, const int* rnorms, unsigned long long* keys,
                       edm_stream_t stream);
int edm_knn_merge(const unsigned long long* keys, int n_lists, long Q, int k, unsigned* dist, int* idx,
                  edm_stream_t stream);
/* Ball membership counts on the same exact distance tile: the one operation that improved precision and recall
 * (Kynkaanniemi et al. 2019, "Improved Precision and Recall Metric for Assessing Generative Models") and density and coverage
 * (Naeem et al. 2020, "Reliable Fidelity and Diversity Metrics for Generative Models") need beyond a k-NN search; the
 * reference has no call site for it.
 * edm_u8_ball_count_partial: queries, refs, qnorms, rnorms, exclude_self, ref_base, splits and the two load paths as in
 *   edm_u8_knn_partial; radii uint32 [R], one closed ball per REFERENCE row, any value up to 2^32 - 1 (d2 < 2^31 is compared
 *   unsigned).  Writes counts int32 [splits][Q]: counts[s][q] = the number of references r in share s with
 *   d2(q, r) <= radii[r], the reference with ref_base + r == q left out when exclude_self is set.  Every element is written
 *   by an ordinary store, an empty share writes 0, and there are no atomics; the total is the caller's integer sum over the
 *   shares (and over the chunks of a chunked call), so it depends on neither.  Limits, status -1 otherwise: 1 <= D <= 32768,
 *   1 <= Q <= 65535 * 128, R >= 1, ref_base >= 0, ref_base + R <= 2^31 - 128, 1 <= splits <= 1024, no null pointers. */
int edm_u8_ball_count_partial(const void* queries, const void* refs, long Q, long R, int D, const unsigned* radii,
                              int exclude_self, long ref_base, int splits, const int* qnorms, const int* rnorms, int* counts,
                              edm_stream_t stream);

/* ---------------------------------------------------------------- ideal denoiser of a training set (csrc/ideal.hip) */
/* D*(x; sigma) = sum_i w_i y_i with w = softmax_i(-|x - y_i|^2 / (2 sigma^2)) over the rows y_i = (u_i / 255 - mean) / std of
 * a resident uint8 set, and per query lse = log sum_i exp(l_i), ent = -sum w_i log w_i, the largest weight and its index (ties
 * to the lower index).  The reference has no call site; Karras et al. 2022 App. B.3.
 * Both products run on the fp32 MFMA (v_mfma_f32_16x16x4_f32) in units of one grey level around 128, where the uint8 side is an
 * exact integer; the logit's three terms meet in fp64; softmax, statistics and the output are fp32 with max subtraction.  No
 * floating-point atomics, every output element leaves by an ordinary store, and with the chunking fixed the bits of a row
 * depend on that row's operands and the reference set alone.  A call walks the reference set in chunks of Rc rows:
 *   begin, then per chunk (logits, softmax, accumulate), then finish; the workspace S is [Q][ld] floats, ld >= Rc.
 * Layouts: x fp32 [Q][K] and refs u8 [R][K] row-contiguous, K = C H W of NCHW; sigma fp32 [Q]; labels int64 [Q] or null;
 * ref_labels int32 [R] or null; qd fp64 [Q][2]; state fp32 [Q][8]; rnorms int32: edm_u8_norms of the rows passed.
 * refs may sit at any byte alignment: 16-byte / 8-byte loads run when x (P for accumulate) and refs are 16-byte aligned and
 * K % 16 == 0, element loads otherwise, with the same results.  Limits, status -1 and nothing launched otherwise:
 * 1 <= K <= 32768, 1 <= Q <= 65535 * 64, 1 <= Rc, ref_base + Rc <= 2^31 - 128, ld >= Rc (accumulate: ld % 4 == 0 and S 16-byte
 * aligned), mean finite, std finite and > 0, num_classes >= 1 with labels.  Status -2: the launch failed.
 * Bad values never index memory: sigma <= 0 or non-finite, a non-finite x row or a class outside [0, num_classes) make that
 * row NaN (top_idx -1), leave the other rows alone and set bit 1 of the health word (as edm_eval_diffuse for a bad level);
 * classes are compared with ref_labels, never used as an index.  No host synchronisation, no host reads: capture-safe.
 * edm_ideal_begin: per query |z|^2 and a^2 / (2 sigma^2) -> qd, the bad flag and the empty running state -> state.
 * edm_ideal_logits: S[q][j] = the logit of query q against row j of the chunk `refs` (u8 [Rc][K]).
 * edm_ideal_softmax: S -> the weights exp(l - running max) in place (a row of another class: 0, taking no part in max, sum or
 *   statistics); state moves on by the chunk.  ref_base: the set index of the chunk's row 0.  Masking needs ref_labels AND
 *   labels; with either null every row takes part.
 * edm_ideal_accumulate: acc[q][k] = alpha_q acc[q][k] + sum_j S[q][j] (refs[j][k] - 128); first != 0: acc is written, not read.
 * edm_ideal_finish: D = acc / (255 std s) + (128 / 255 - mean) / std (D may be acc), lse / ent / top_w fp32 [Q], top_idx
 *   int32 [Q]; sets the health bit on a non-finite output too. */
int edm_ideal_begin(const float* x, const float* sigma, const long long* labels, int num_classes, long Q, int K, float mean,
                    float stdv, double* qd, float* state, unsigned* health, edm_stream_t stream);
int edm_ideal_logits(const float* x, const void* refs, const int* rnorms, const double* qd, long Q, long Rc, int K,
                     float mean, float stdv, float* S, long ld, edm_stream_t stream);
int edm_ideal_softmax(float* S, long ld, long Q, long Rc, long ref_base, const int* ref_labels, const long long* labels,
                      float* state, edm_stream_t stream);
int edm_ideal_accumulate(const float* P, long ld, const void* refs, const float* state, long Q, long Rc, int K, int first,
                         float* acc, edm_stream_t stream);
int edm_ideal_finish(const float* acc, const float* state, long Q, int K, float mean, float stdv, float* D, float* lse,
                     float* ent, float* top_w, int* top_idx, unsigned* health, edm_stream_t stream);

/* ---------------------------------------------------------------- moments and polynomial-kernel sums in fp64 (csrc/moments.hip) */
/* The two reductions behind the Frechet distance of two sample sets (Heusel et al. 2017, "GANs Trained by a Two Time-Scale
 * Update Rule Converge to a Local Nash Equilibrium"; the distance itself: Dowson & Landau 1982, "The Frechet distance between
 * multivariate normal distributions") and the kernel inception distance (Binkowski et al. 2018, "Demystifying MMD GANs");
 * the reference has no call site for either.  Both run on v_mfma_f64_16x16x4_f64 over rows that are converted to fp64 as
 * they are loaded: no fp64 copy of a set is made.  dtype: 0 = uint8, 1 = float32.  uint8 moments and dot products are exact
 * integers in fp64 (every sum stays below 2^53), so they do not depend on tiling or split count; float32 products are exact
 * and the sums round in an order fixed by the arguments, so two calls give the same bits.  No atomics; every partial is
 * written by an ordinary store.  Sets are row-contiguous at any byte alignment: aligned vector loads when the base is
 * 16-byte aligned and a row is a whole number of them (moments: D % 4 == 0; sums: D % 16 == 0 for uint8, D % 4 == 0 for
 * float32), element loads otherwise, same results.  Index lists are trusted:
 * the caller checks that every entry names a row of its set.  Status -1 and nothing launched on a bad argument.
 * edm_moments_splits: the number of shares of the N axis the library would give an N x D set (host logic only).
 * edm_moments_partial: x [rows][D]; index long [N] (may be null: rows 0 .. N - 1; may repeat rows, any order) gathers the N
 *   rows that take part; shift double [D] (may be null) is subtracted from every row in fp64 before the products (the second
 *   pass of a two-pass covariance; null keeps uint8 results exact integers).  Share s of `splits` (the caller's choice in
 *   [1, 1024]) takes rows N s / splits .. N (s + 1) / splits and writes psum [splits][D] and, of pgram [splits][D][D], the
 *   64 x 64 tiles on and above the tile diagonal (entries with i / 64 > j / 64 are not written).  pgram null: the column
 *   sums only.  Limits: 1 <= N < 2^40, 1 <= D <= 32768.
 * edm_moments_finish: sum [D] and gram [D][D] (both null together with pgram) = the partials added in split order, the upper
 *   triangle mirrored into the lower.
 * edm_poly_sums_partial: for each of S subsets, rows idx_a[s][0 .. ma) of a and idx_b[s][0 .. mb) of b (long [S][ma] and
 *   [S][mb]; a null list: rows 0 .. m - 1 for every subset): partial[s][ti][tj] = the sum over the 64 x 64 tile (ti, tj) of
 *   the ma x mb pairs of (gamma a_i . b_j + coef0)^degree, the power by repeated multiplication, degree in [1, 4].
 *   exclude_equal_index skips the pairs whose two row numbers are equal (by number, not by value: a duplicate row still
 *   counts).  partial double [S][ceil(ma / 64)][ceil(mb / 64)].  Limits: 1 <= S <= 65535, 1 <= ma, mb <= 65535 * 64,
 *   1 <= D <= 2^24.
 * edm_poly_sums_finish: sums [S] = the `tiles` partials of each subset, added in a fixed order. */
int edm_moments_splits(long N, int D);
int edm_moments_partial(const void* x, int dtype, const long* index, long N, int D, const double* shift, int splits,
                        double* psum, double* pgram, edm_stream_t stream);
int edm_moments_finish(const double* psum, const double* pgram, int splits, int D, double* sum, double* gram,
                       edm_stream_t stream);
int edm_poly_sums_partial(const void* a, int dtype_a, const long* idx_a, const void* b, int dtype_b, const long* idx_b, int S,
                          long ma, long mb, int D, double gamma, double coef0, int degree, int exclude_equal_index,
                          double* partial, edm_stream_t stream);
int edm_poly_sums_finish(const double* partial, int S, long tiles, double* sums, edm_stream_t stream);

/* ---------------------------------------------------------------- feature-space nearest neighbours (csrc/neighbors_f32.hip) */
/* The float32 form of the exact search above, for the feature spaces in which precision and recall (Kynkaanniemi et al.
 * 2019) and density and coverage (Naeem et al. 2020) were defined; the reference has no call site for it.  Distances are
 * fp64 on v_mfma_f64_16x16x4_f64 (the tile engine of the moments above): d2 = fmax((|q|^2 + |r|^2) - 2 q.r, 0), float32
 * products exact, only the sums round.  The bits of d2(q, r) depend on the two rows and D only -- not on tile position,
 * splits, chunking, the load path (16-byte loads when a base is 16-byte aligned and D % 4 == 0, element loads otherwise) or
 * on which kernel computes them -- and identical rows give +0.0 exactly.  The order is the pair (bit pattern of d2 as
 * uint64, reference index), ties to the lower index.  No atomics; every output element is written by an ordinary store.
 * Input must be finite (the caller's check).  Limits, status -1 otherwise: 1 <= k <= 32, k <= R (k <= R - 1 with
 * exclude_self) unless partial, 1 <= D <= 32768, Q <= 65535 * 64, ref_base + R <= 2^31 - 64, 1 <= splits <= 1024.
 * edm_f32_knn_splits: the number of shares of the R axis the library would give a Q x R search (host logic only).
 * edm_f32_norms: norms fp64 [n_rows] = |x|^2 with the bits of the distance tile's x.x (the tile run on the rows against
 *   themselves, the diagonal kept); the qnorms / rnorms of the two calls below.
 * edm_f32_knn_partial: writes keys_d2 uint64 [splits][Q][k] (bit patterns of d2) and keys_idx int32 [splits][Q][k]
 *   (ref_base + reference row), each list ascending, unused slots (all-ones, -1).  Arguments as in edm_u8_knn_partial.
 * edm_fknn_merge: n_lists lists per query (splits of one call or of every chunk, end to end) -> dist fp64 [Q][k],
 *   idx int32 [Q][k], ascending by (d2, idx).
 * edm_f32_ball_count_partial: counts int32 [splits][Q], counts[s][q] = the number of references r in share s with
 *   d2(q, r) <= radii[r] (closed compare in fp64; radii fp64 [R], finite and >= 0); an empty share writes 0 and the caller
 *   adds the shares as integers.  Arguments as in edm_u8_ball_count_partial. */
int edm_f32_knn_splits(long Q, long R);
int edm_f32_norms(const void* x, long n_rows, int D, double* norms, edm_stream_t stream);
int edm_f32_knn_partial(const void* queries, const void* refs, long Q, long R, int D, int k, int exclude_self, long ref_base,
                        int partial, int splits, const double* qnorms, const double* rnorms, unsigned long long* keys_d2,
                        int* keys_idx, edm_stream_t stream);
int edm_fknn_merge(const unsigned long long* keys_d2, const int* keys_idx, int n_lists, long Q, int k, double* dist, int* idx,
                   edm_stream_t stream);
int edm_f32_ball_count_partial(const void* queries, const void* refs, long Q, long R, int D, const double* radii,
                               int exclude_self, long ref_base, int splits, const double* qnorms, const double* rnorms,
                               int* counts, edm_stream_t stream);

/* ---------------------------------------------------------------- denoiser activations as features (csrc/features.hip) */
/* Global average pool of an fp32 NHWC activation into a slice of a feature row (Xiang et al. 2023, "Denoising Diffusion
 * Autoencoders are Unified Self-supervised Learners": pooled activations of an intermediate block; the reference has no
 * call site for it).  x fp32 [B][HW][C] contiguous; row b of out starts at out + b * out_stride (floats) and only its columns
 * [out_offset, out_offset + C) are written: out[b][out_offset + c] = (float)((sum_p (double)x[b][p][c]) / (double)HW).
 * The sum is fp64 in an order that depends on HW alone (pixel p in slot p % 32, slots in ascending order), so a row's
 * bits depend on neither B, its place in the batch, C nor the load path (16-byte loads when C % 4 == 0 and x is 16-byte
 * aligned, element loads otherwise).  No atomics.  Any C >= 1 up to 65535 * 32, any HW >= 1, any B >= 1 (beyond 65 535
 * too); the destination needs 4-byte alignment only; out_stride >= out_offset + C.  Status -1 otherwise. */
int edm_f32_pool_features(const float* x, float* out, int B, int HW, int C, long out_stride, int out_offset,
                          edm_stream_t stream);

/* ---------------------------------------------------------------- optimised sampling schedules (csrc/schedule.hip) */
/* The local error of every single-step jump between two nodes of a recorded teacher trajectory: the pair costs of the
 * dynamic-programming schedule search (Watson et al. 2021; Chen et al. 2024; the reference has no call site for it).
 * X fp32 [G+1][B][K], node-major: the states at the grid nodes, node G the result; S fp32 [G][B][K]: the Euler slopes at
 * nodes 0 .. G-1; tau: DEVICE fp64 [G+1], the grid (the fp32 table values widened), tau[G] = 0; d2: DEVICE fp64
 * [B][G][G+1], every entry WRITTEN.  For i < j, with h = tau[j] - tau[i] and everything in fp64:
 *   order 1, and order 2 when j == G (Heun's closing step is Euler-only):  e_k = x_ik + h s_ik - x_jk
 *   order 2 when j < G (the trapezoid along the trajectory):              e_k = x_ik + (h/2)(s_ik + s_jk) - x_jk
 *   d2[b][i][j] = sum_k e_k^2,
 * evaluated as e = fma(c h, s_i + s_j', x_i - x_j), (c, s_j') = (1/2, s_j) or (1, 0).  Entries with j <= i are +0.0.
 * The bits of d2[b][i][j] depend only on K, the two nodes' rows of sample b, tau[i], tau[j] and order: not on B, G, the
 * pair's place in a tile, the other pairs or the load path (dwordx4 when K % 4 == 0 and X, S are 16-byte aligned, the same
 * quads element by element otherwise).  No floating-point atomics: thread t of 256 adds the quads t, t + 256, ... of the K
 * axis in ascending order, then the wave butterfly and the four wave totals in index order, a function of K alone.
 * Any K >= 1, any B >= 1 with B * ceil(G/4) * ceil((G+1)/8) < 2^31, 1 <= G <= EDM_SCHEDULE_MAX_GRID, order 1 or 2; tau and
 * d2 8-byte aligned.  Status -1 otherwise. */
#define EDM_SCHEDULE_MAX_GRID 256
int edm_pair_step_errors(const float* X, const float* S, const double* tau, int B, int G, long K, int order, double* d2,
                         edm_stream_t stream);

/* ---------------------------------------------------------------- feature clustering (csrc/kmeans.hip) */
/* The update half of a Lloyd iteration (k-means on features: Hu et al. 2023, "Self-guided diffusion models"; the reference
 * has no call site for it): per cluster, the column sums of its member rows in fp64, each float32 widened as it is loaded,
 * through an inverted index.  The assignment half is edm_f32_knn_partial with k = 1.
 * The order.  Cluster k's rows are listed in ascending row number; the row at position p of that list is in chunk
 * p / EDM_CLUSTER_BLOCK.  partial(chunk) = (((+0.0 + row_0) + row_1) + ...) over the chunk's rows in ascending position;
 * sums[k] = (((+0.0 + partial_0) + partial_1) + ...) over the cluster's chunks in ascending chunk number.  d2sums follows
 * the same sequence on d2[row].  The bits of an output element are a function of the cluster's member list (and the
 * values) alone: not of K, n, the other clusters, the grid, or the load path (16-byte loads when D % 4 == 0 and x is
 * 16-byte aligned, element loads otherwise).  No atomics; a cluster without members gets +0.0.
 * edm_cluster_block: EDM_CLUSTER_BLOCK as the library was built (host logic only): the caller cuts its chunk tables with
 *   this value, so a library built with another chunk length stays consistent with its callers.
 * edm_f32_cluster_sums_partial: x float32 [n][D] row-contiguous, 4-byte aligned; members int32 [n]: the rows of cluster 0
 *   ascending, then cluster 1, ...; starts int32 [K+1]: cluster k owns members[starts[k] .. starts[k+1]); chunk_first int32
 *   [K+1]: cluster k owns the chunks chunk_first[k] .. chunk_first[k+1], ceil(its members / EDM_CLUSTER_BLOCK) of them;
 *   chunk_cluster int32 [n_chunks]; d2 fp64 [n] or null.  Writes partial fp64 [n_chunks][D] and, with d2, partial_d2 fp64
 *   [n_chunks]: the whole workspace is n_chunks (D + 1) <= (n / EDM_CLUSTER_BLOCK + K)(D + 1) doubles.  The tables are
 *   the caller's responsibility (every member a row number in [0, n)).
 * edm_f32_cluster_sums_finish: sums fp64 [K][D] and, when partial_d2 and d2sums are given, d2sums fp64 [K]; every element
 *   written.
 * Limits, status -1 otherwise: 1 <= n <= 2^31 - 64, 1 <= D <= 32768, 1 <= K <= 2^20, 1 <= n_chunks <= n /
 * EDM_CLUSTER_BLOCK + K. */
#ifndef EDM_CLUSTER_BLOCK
#define EDM_CLUSTER_BLOCK 64
#endif
int edm_cluster_block(void);
int edm_f32_cluster_sums_partial(const void* x, const int* members, const int* starts, const int* chunk_first,
                                 const int* chunk_cluster, const double* d2, long n, int D, int K, long n_chunks,
                                 double* partial, double* partial_d2, edm_stream_t stream);
int edm_f32_cluster_sums_finish(const double* partial, const double* partial_d2, const int* chunk_first, int D, int K,
                                double* sums, double* d2sums, edm_stream_t stream);

/* ---------------------------------------------------------------- paired image quality (csrc/quality.hip) */
/* SSIM and the squared error of image i against image i (Wang, Bovik, Sheikh, Simoncelli 2004; the reference has no call
 * site for it).  a, b: n images of C channels, H x W, both uint8 (is_u8) or both float32 in pixel units; element (i, c, y,
 * x) of a sits at a + i strides_a[0] + c strides_a[1] + y strides_a[2] + x strides_a[3] (HOST arrays of 4 element strides,
 * >= 0), so uint8 NHWC and float32 NCHW go through one kernel without a copy.  window: DEVICE fp64 [win], the 1-D taps as
 * the host built them (the same bits as the reference uses); win odd, 3 <= win <= 15, win <= min(H, W).  data_range L:
 * C1 = (0.01 L)^2, C2 = (0.03 L)^2.  Per image and channel, in fp64 throughout: the five separably filtered maps mu_a,
 * mu_b, E[a^2], E[b^2], E[ab] over the VALID region (window centres at least (win - 1) / 2 from every edge, no padding),
 *   S = (2 mu_a mu_b + C1)(2 cov + C2) / ((mu_a^2 + mu_b^2 + C1)(var_a + var_b + C2))     (biased variances),
 * ssim fp64 [n][C] = the mean of S; sse fp64 [n][C] = sum (a - b)^2 over the counted pixels (uint8: an exact integer below
 * 2^53); counts int32 [n][2] = (counted pixels, counted window centres).  region: uint8 [n][H][W], or [1][H][W] with
 * region_shared, or null = everything counted; non-zero = counted.  sse runs over counted pixels, the mean over valid
 * centres that are themselves counted (the windows still read every pixel); no counted centre: counts[i][1] = 0 and NaN.
 * The order.  The valid region is cut into tiles of 16 x 32 centres from its corner (edm_pair_ssim_tiles of them, a
 * function of (H, W, win)).  In a tile, thread t of 256 adds its centres t, t + 256 (row-major in the tile) in ascending
 * order, then a halving tree over the threads; the tiles are added in row-major tile order.  A tile owns the pixels of
 * its 16 x 32 block (the last tile row / column also the halo behind it) for sse, same order.  The bits of row i depend
 * on that image pair, the shape, the window and the region row alone: not on n, the row's place or the strides.  No
 * atomics; every output element is one ordinary store.  partial: workspace fp64 [n C tiles][4].
 * Limits, status -1 otherwise: H W < 2^31, n C tiles < 2^31 (launched in chunks of 2^23 workgroups, which changes no bit).
 * edm_pair_ssim_tiles: the tiles of one plane (host logic only); 0 for a window the library refuses. */
long edm_pair_ssim_tiles(int H, int W, int win);
int edm_pair_ssim(const void* a, const void* b, int is_u8, long n, int C, int H, int W, const long* strides_a,
                  const long* strides_b, const double* window, int win, double data_range, const unsigned char* region,
                  int region_shared, double* partial, double* ssim, double* sse, int* counts, edm_stream_t stream);
/* The LPIPS form of a distance between two sets of activations (Zhang et al. 2018, without its learned linear layers and
 * with the project's own denoiser in the place of VGG / AlexNet: NOT LPIPS; the reference has no call site for it).
 * a, b fp32 [B][HW][C] contiguous (NHWC maps of one tap).  Row b of out starts at out + b * out_stride (doubles) and only
 * its element `column` is written:
 *   out[b][column] = (1 / HW) sum_p sum_c (a_pc / (|a_p| + 1e-10) - b_pc / (|b_p| + 1e-10))^2       in fp64,
 * in the two-pass form per pixel (the norms, then the squared differences of the scaled values, x * (1 / (|x| + 1e-10)),
 * each product rounded before the subtraction), never 2 - 2 cos: identical inputs give exactly +0.0; an all-zero pixel vector gives 0 / 1e-10 = 0.
 * The order, a function of (HW, C) alone.  One wave per pixel: lane l adds the channels of its quads l, l + 64, l + 128
 * in ascending order, then the xor butterfly (32, 16, .. 1).  Wave w of 8 adds the pixels w, w + 8, ... in ascending
 * order; the 8 wave totals are added in ascending order and divided by HW once.  Row b depends on neither B, its place
 * nor the load path (16-byte loads when C % 4 == 0 and a, b are 16-byte aligned, element loads otherwise).  No atomics.
 * Limits, status -1 otherwise: 1 <= C <= 768 (a pixel row of each map stays in one wave's registers), 0 <= column <
 * out_stride. */
int edm_f32_pair_feature_distance(const float* a, const float* b, double* out, int B, int HW, int C, long out_stride,
                                  int column, edm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TINYEDM_HIP_H */
