// conv_args.hpp — kernel argument block, device helpers and launcher declarations shared by the convolution kernels: conv_mfma.hip (which
// dispatches to the others), conv_rows.hip, conv_pw.hip, conv_k3d.hip, rtdetr_ops.hip, and — through rows16_parts.hpp — conv_rows16.hip,
// conv_rows16pc.hip and conv_trunk.hip.
#pragma once
#include "conv_route.hpp"
#include "dw_bound.hpp"
#include "ops.hpp"

namespace ffp {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

struct ConvArgs {
  const void* in;
  const void* wpk;
  const float* bias;
  void* out;
  const void* res1;
  const void* res2;
  const int4* in_tab;
  const int4* out_tab;
  const int4* tiles;
  long long total_px;   // KS == 1: flat pixel count
  int in_cs, in_coff, cin, cin_pad;
  int out_cs, out_coff, cout;
  int r1_cs, r1_coff, r2_cs, r2_coff;
  float s1, s2;
  int act_post;         // activation applied after the residual terms (SCRFD: Relu(Add(conv, x))); ACT_NONE for every other plan
  int act, out_f32, up, n_nblk, ncg, ntiles32, vec_ok, fast_out;
  int force_shape;   // ConvOp::force_shape; no kernel and no launcher reads it (the slot keeps the argument block's layout)
  int dbg;   // tuning only (ffp_op_conv2d_time): 1 skip stores, 2 skip MFMAs, 4 skip chunk refetch, 8 skip LDS stash
  const void* up_src;  // 1x1 only: channels [0, up_c) come from this coarser view through up_map (see ConvOp::has_up2)
  const int* up_map;
  int up_c, up_cs;
  const void* zeros;   // 256 zero bytes in device memory (padding source of the LDS-DMA loader in conv_rows.hip)
  // scaled split (FFP_PREC_F32X3): the loader multiplies the activations by 2^(13 - e), e = exponent of max(*amax_in, *amax_in2),
  // before cutting them into fp16 hi + lo parts; the weights were packed with a per-output-channel power of two (oscale = its
  // inverse); the epilogue multiplies the sums back and raises *amax_out to the largest |output| it stores
  const unsigned* amax_in;
  const unsigned* amax_in2;
  unsigned* amax_out;
  const float* oscale;
  // per-image exponent slots (TView::amax_n > 1): slot of image i = amax_*[i]; amax_img = 0: one slot per buffer (index 0 for every image).
  // 3x3 kernels know the image of a tile; the 1x1 kernels look the image of a 32-pixel fragment of the flat pixel array up in frag_img
  // (levels aligned to 32 pixels: no fragment straddles two images)
  int amax_img;
  const int* frag_img;                 // [fragment] x {image, end of the image's real pixels}
  int ntiles_host;          // tile-loop kernels (conv_rows16.hip): tiles of an exact-mode launch (the grid no longer says)
  const int* n_tiles_dev;   // capacity-mode levels (Level::reserve): the batch's tile count lives in device memory and the grid is
                            // sized for the capacity — workgroups past n_tiles * n_nblk exit; nullptr: the grid is exact
  // stem-fused loader (conv_mfma_kernel<..., STEM = true>, launch_stem_conv): the conv's input is never stored — every workgroup
  // computes its halo tile of the image-input conv (model.0: 3x3 stride 2 + SiLU over the letterboxed u8 frame) on the matrix
  // cores and writes it straight into the LDS stage as split fp16 records
  const unsigned char* st_frame;     // HxWx3 u8
  const LetterboxImg* st_imgs;       // per item
  const int4* st_tab;                // level table of the letterboxed network images (.y rows, .z columns)
  const void* st_w;                  // stem weights as MFMA A fragments [chunk][hi|lo][64 lanes] x 16 B (stem_pack_kernel)
  const float* st_bias;
  int st_W;                          // frame width
  long long st_bytes;                // frame size in bytes, rounded up to whole dwords (range check of the loader's dword reads)
  float st_scale;                    // 1 / (power of two the packed stem weights were multiplied by)
  const int* gate;                   // ConvOp::gate: the 3x3 launchers pick the gated tile table (no 3x3 kernel reads it); the 1x1 kernels read it per fragment (frag_img)
};

// (logical workgroup id, number of live workgroups) for a tile kernel; live == 0: this workgroup has nothing to do
__device__ __forceinline__ int live_workgroups(const ConvArgs& a) {
  return a.n_tiles_dev ? __builtin_amdgcn_readfirstlane(*a.n_tiles_dev) * a.n_nblk : (int)gridDim.x;
}

__device__ __forceinline__ int xcd_remap(int b, int nwg) {
  // blocks b and b+8 share an XCD (observed round-robin dispatch): give each XCD a contiguous run of logical ids.
  const int xcd = b & 7, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
}

// wave-uniform 32-bit load through the scalar cache: read-only tables and max-|value| slots written by EARLIER kernels. (Inside a
// loop with stores hipcc turns a uniform global load into a vector load + readfirstlane, i.e. a full memory round trip on the
// critical path; the constant address space keeps it an s_load whose result nothing waits for until it is used.)
__device__ __forceinline__ int sload(const void* p, int idx) {
  typedef const __attribute__((address_space(4))) int* cptr;
  return reinterpret_cast<cptr>(reinterpret_cast<unsigned long long>(p))[idx];
}

// wave-wide maximum of non-negative, non-NaN floats as a wave-uniform bit pattern: four DPP steps inside the rows of 16 lanes,
// then the four rows by v_readlane (no LDS round trips, unlike __shfl_xor)
__device__ __forceinline__ unsigned wave_max_bits(float mx) {
  int v = __float_as_int(mx);
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true));     // quad_perm [1,0,3,2]
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true));     // quad_perm [2,3,0,1]
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true));    // row_half_mirror
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true));    // row_mirror
  const int a = max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16));
  const int b = max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48));
  return (unsigned)max(a, b);
}

// raise a max-|value| slot (see TView::amax): wave-wide maximum first, and the atomic only when it would change the slot.
// `old` = a value the slot held at some earlier time (slots only grow, so a stale value costs at most a redundant atomic): kernels that
// raise a slot per work item load it early so that nothing waits for the round trip here.
__device__ __forceinline__ unsigned slot_peek(const unsigned* slot) {
  return __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void raise_amax(unsigned* slot, float mx, unsigned old) {
  const unsigned b = wave_max_bits(mx);
  if ((threadIdx.x & 63) == 0 && b > old) atomicMax(slot, b);
}
__device__ __forceinline__ void raise_amax(unsigned* slot, float mx) {
  const unsigned b = wave_max_bits(mx);
  if ((threadIdx.x & 63) == 0 && b > slot_peek(slot)) atomicMax(slot, b);
}

// bit pattern of max |value| of the conv's input for image `img` (both sources of a two-source 1x1)
__device__ __forceinline__ unsigned amax_in_bits(const ConvArgs& a, int img) {
  if (!a.amax_in) return 0u;
  const int i = a.amax_img ? img : 0;
  unsigned m = a.amax_in[i];
  if (a.amax_in2) m = max(m, a.amax_in2[i]);
  return m;
}
// the same through the scalar cache (img wave-uniform)
__device__ __forceinline__ unsigned amax_in_bits_s(const ConvArgs& a, int img) {
  if (!a.amax_in) return 0u;
  const int i = a.amax_img ? img : 0;
  unsigned m = (unsigned)sload(a.amax_in, i);
  if (a.amax_in2) m = max(m, (unsigned)sload(a.amax_in2, i));
  return m;
}

// activation scale of the split and its inverse from a max-|value| bit pattern: 2^(13 - e) puts the largest value in [2^13, 2^14)
__device__ __forceinline__ void split_scales(unsigned amax_bits, float* t, float* tinv) {
  split_scales_hd(amax_bits, t, tinv);            // dw_bound.hpp: the one text of this step, host and device (dw_bound_host_check.cpp runs it on the CPU)
}

// (x0, x1) * t -> packed fp16 pair hi = RN(x * t) and packed fp16 pair lo = RN(x * t - hi), t a power of two: the operand split of
// FFP_PREC_F32X3. v_fma_mix{lo,hi}_f16 compute an fp32 fma and round once to fp16, reading the fp16 third operand in place: two
// instructions per value, against four for multiply / convert / convert back / subtract / convert. Bit-identical to
//   hi = (_Float16)(x * t); lo = (_Float16)fmaf(x, t, -(float)hi)
// on every input (tools/mix_split_check.hip compares 50 M values over all exponents, fp16 overflow and subnormal results).
__device__ __forceinline__ void split_pair(float x0, float x1, float t, unsigned& hi, unsigned& lo) {
  unsigned h, l;                        // mixlo leaves the upper half of its destination as it was; mixhi then writes it
  asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(h) : "v"(x0), "v"(t));
  asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(h) : "v"(x1), "v"(t));
  asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]" : "=v"(l) : "v"(x0), "v"(t), "v"(h));
  asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(l) : "v"(x1), "v"(t), "v"(h));
  hi = h;
  lo = l;
}

// the activations with IEEE expf and divide: the depthwise and image-input kernels (ops_misc.hip) and the depthwise sums conv_dwpw.hip computes in
// its loader, which must have the bits dwconv3x3_col_kernel stores
__device__ __forceinline__ float act_fn(float v, int act) {
  if (act == ACT_SILU) return v / (1.0f + expf(-v));
  if (act == ACT_LRELU) return v >= 0.f ? v : v * 0.2f;
  if (act == ACT_RELU) return fmaxf(v, 0.f);
  return v;
}

__device__ __forceinline__ float apply_act(float v, int act) {
  // SiLU with the hardware exp2 / rcp (1 ulp each): ~6 VALU ops instead of ~25 for expf + IEEE divide; the epilogue of a
  // 256 px x 64 ch block otherwise spends ~2.7 us in the activation alone
  if (act == ACT_SILU) return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v));
  if (act == ACT_LRELU) return v >= 0.f ? v : v * 0.2f;
  if (act == ACT_RELU) return fmaxf(v, 0.f);
  return v;
}

// Raw BUFFER loads of conv_mfma, conv_rows and the rows16 family (conv_k3d keeps lambdas of its own: these in their place moved all its streams): the resource base is wave-uniform
// (readfirstlane'd halves: SGPRs), the per-lane part a 32-bit byte offset; a lane with nothing to read or write uses BUF_OOB, which the range check turns into zeros / a dropped store.
constexpr unsigned BUF_OOB = 0xFFFFFFFFu;
__device__ __forceinline__ auto buf_rsrc(const unsigned char* p, unsigned bytes = 0x7FFFFFF0) {
  const unsigned long long u = reinterpret_cast<unsigned long long>(p);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
  return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<unsigned char*>(((unsigned long long)hi << 32) | lo), 0, bytes, 0x00020000);
}
typedef decltype(buf_rsrc(nullptr)) buf_rsrc_t;
__device__ __forceinline__ uint4 buf_load16(buf_rsrc_t rs, unsigned off, int soff = 0) {      // soff: wave-uniform byte offset (an SGPR operand, no VALU)
  const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, off, soff, 0);
  return make_uint4(v[0], v[1], v[2], v[3]);
}
// ---- host: what a kernel family's epilogue implements of the ConvOp contract (ops.hpp: act -> v * s1 + res1 -> v * s2 + res2 -> act_post), stated once next
// to the kernel (true to the kernel text, not to today's callers), and the one check every eligibility predicate starts from
struct EpiCaps { unsigned acts; bool res, act_post, out_f16, out_f32; };   // acts: bit per Act code applied as `act`; res: res1 / res2 terms; output element types
constexpr unsigned EPI_ALL_ACTS = 1u << ACT_NONE | 1u << ACT_SILU | 1u << ACT_LRELU | 1u << ACT_RELU;
inline bool epilogue_fits(int act, bool res, int act_post, DType out, const EpiCaps& caps) {
  return act >= 0 && act < 32 && (caps.acts >> act & 1u) && (!res || caps.res) && (!act_post || caps.act_post) && (out == F16 ? caps.out_f16 : caps.out_f32);
}
inline bool epilogue_fits(const ConvOp& op, const EpiCaps& caps) { return epilogue_fits(op.act, op.has_res1 || op.has_res2, op.act_post, op.out.dt, caps); }

// host side. Which of these kernels runs an op is decided in conv_route.cpp alone: the predicates below say only whether the kernel CAN run the
// op (at the given shape number) — its layout, geometry and epilogue — and never look at ConvOp::force_shape or the environment.
ConvArgs make_conv_args(const ConvOp& op);
// the generic kernel (conv_mfma.hip), shapes SHAPE_WIDE..SHAPE_NARROW1_H: the shapes that fit the op, the heuristic's pick among them
unsigned conv_generic_mask(const ConvOp& op, const ConvArgs& a);
int conv_generic_choose(const ConvOp& op, const ConvArgs& a);
void launch_conv_generic(ConvArgs& a, int shape, const ConvOp& op, hipStream_t st);
// k3 s1 fp16 row-reuse kernel (conv_rows.hip), shapes SHAPE_ROWS..SHAPE_ROWS_2TILE
bool conv_rows_eligible(const ConvOp& op, const ConvArgs& a, int shape);
void launch_conv_rows(ConvArgs& a, int shape, Level* out_lvl, hipStream_t st);
void conv_rows_init();
// k3 s1 fp16, second generation on v_mfma_f32_16x16x32_f16 (conv_rows16.hip): SHAPE_ROWS16, and SHAPE_ROWS16_RES with the channel block's weights resident in LDS
bool conv_rows16_eligible(const ConvOp& op, const ConvArgs& a, int shape);
void launch_conv_rows16(ConvArgs& a, int shape, const PackedConv& pc, Level* out_lvl, hipStream_t st);
void conv_rows16_init();
unsigned rows16_grid(int n_tiles, int n_nblk, int min_ws, int tcap, const char* what);      // launch extent 8 x Ws of the item dealing (conv_rows16.hip), checked
// the same convs (conv_rows16_eligible) with producer / consumer waves (conv_rows16pc.hip), SHAPE_ROWS16PC: opt-in (measured 0.73-0.94x); bit-identical results
void launch_conv_rows16pc(ConvArgs& a, const PackedConv& pc, Level* out_lvl, hipStream_t st);
void conv_rows16pc_init();
// 1x1 fp32-split convs without LDS staging of the activations (conv_pw.hip): shape_bit(s) of the mask = shape s (SHAPE_PW_*) can run this op
unsigned conv_pw_mask(const ConvOp& op, const ConvArgs& a);
void launch_conv_pw(ConvArgs& a, int shape, hipStream_t st);
void conv_pw_init();

// a depthwise 3x3 + activation inside the loader of a 1x1 fp32-split conv to 128 channels, optionally with a closing 1x1 to <= 4 channels in the
// epilogue (conv_dwpw.hip, ConvOp::dw / ConvOp::fin): one shape (SHAPE_DWPW). The launcher builds its own argument block from the op.
bool conv_dwpw_eligible(const ConvOp& op, bool need_storage = true);      // need_storage = false: views without storage yet (a plan asking before it allocates)
void launch_conv_dwpw(const ConvOp& op, hipStream_t st);
void conv_dwpw_init();

// 3x3 fp32-split convs, stride 1 and 2, weights straight from L2 into MFMA operand registers (conv_k3d.hip): shape_bit(s) of the mask =
// shape s (SHAPE_K3D_*) can run this op; results are bit-identical to the generic kernel's
unsigned conv_k3d_mask(const ConvOp& op, const ConvArgs& a);
void launch_conv_k3d(ConvArgs& a, int shape, int stride, Level* out_lvl, hipStream_t st);
void conv_k3d_init();

}  // namespace ffp
