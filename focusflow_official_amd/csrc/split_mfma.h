// Device helpers shared by the split-MFMA kernels (gfx950 only): ONE definition of every convention that lets a layer compute
// the same bits whichever kernel runs it (tests/test_hip_split.py) - the lane-to-pixel map, the slot
// orders, the term order of the three-term product and the fragment-order weight image.  The split format itself (scales, ff::split4 / split_pair4, the split-pair stores) is ff_common.h's.
// Where two kernels need different machine code for the same piece, the difference is a named template parameter here.
#pragma once
#include "ff_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) char* lds_ptr_t;      // (unsigned)(unsigned long)(lds_ptr_t)p = p's LDS byte address
typedef __attribute__((address_space(1))) const void* gptr_t;   // operands of __builtin_amdgcn_global_load_lds
typedef __attribute__((address_space(3))) void* lptr_t;

namespace ff {

// a buffer offset no descriptor covers (every tensor is below 2 GiB), and + any soffset < 2^31 stays below 2^32: the range
// check sees it out of range -> loads give zeros, stores are dropped
constexpr unsigned OOB = 0x7fffffffu;

// ---- v_mfma_f32_16x16x32_f16 lane layout: lane = (row i = lane & 15, k-group g = lane >> 4).  A ds_read_b128 serves lanes
// {0-3, 12-15} of one k-group together with {4-11} of the next: MFMA rows 4..11 take the even positions of a 16-row tile (a
// pixel's column, a weight row's place in LDS), rows 0..3 / 12..15 the odd ones - different halves of the 64 banks.
__device__ __forceinline__ int PI16(int i) { return (i >= 4 && i < 12) ? 2 * (i - 4) : (i < 4 ? 2 * i + 1 : 2 * (i - 12) + 9); }
// place of k-group g inside a term's 64 bytes where the rows are pitched, not swizzled: the 16-byte groups sit in the order 0, 2, 1, 3
__device__ __forceinline__ int KG16(int g) { return ((g & 1) << 1) | (g >> 1); }
// XOR slot swizzle of the 128-byte LDS rows: 16-byte piece -> slot of row `row`
__device__ __forceinline__ int swz(int row, int piece) { return piece ^ ((row >> 1) & 7); }

// ---- LDS by byte address, LDS-DMA
template <typename T>
__device__ __forceinline__ T lds_ld(unsigned addr) { return *(__attribute__((address_space(3))) const T*)(unsigned long)addr; }
__device__ __forceinline__ f16x8 lds_ld16(unsigned addr) { return lds_ld<f16x8>(addr); }
template <int N>
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// one LDS-DMA piece: 64 lanes x 16 bytes -> 1 KB at LDS address `dst` (M0), source = rsrc base + voff + soff.
// UNIFORM: dst and soff go through readfirstlane first - they are uniform values, but when the scalar registers run short the
// allocator parks them in a vector register, which these operands do not take (conv_dma.hip).  A kernel that never ran short
// (gru_pass.hip) passes false: the copies change its scalar code.
template <bool UNIFORM>
__device__ __forceinline__ void dma_piece(unsigned voff, __amdgpu_buffer_rsrc_t rs, unsigned dst, unsigned soff) {
    unsigned keep;
    if (UNIFORM) {
        dst = (unsigned)__builtin_amdgcn_readfirstlane((int)dst);
        soff = (unsigned)__builtin_amdgcn_readfirstlane((int)soff);
    }
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                 "buffer_load_dwordx4 %1, %2, %4 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(rs), "s"(dst), "s"(soff)
                 : "memory");
}

// ---- the three-term product.  x w ~ (x0 w0 + x0 w1 + x1 w0) / (sx sw), summed into ONE fp32 accumulator in the order
//   w0 x0,  w1 x0,  w0 x1
// per K chunk.  fp32 addition does not associate: every kernel that may run a layer must add the terms in this order, or the
// layer's bits depend on its route.  TERMS = 1 keeps w0 x0 only (plain fp16 operands).  The weight pair (w0, w1) is the A operand;
// W_IS_B says it is the B operand (the kernels whose MFMA rows are pixels) - same terms, same order.
// Operands come as the MFMA takes them: the A pair (a0, a1), then the B pair (b0, b1) - f16x8, or the 16 bytes as they were
// loaded (an f32x4 register set).
#define FF_MFMA_TERMS(name_, acc_t_, mfma_)                                                                                      \
    template <int TERMS, bool W_IS_B = false, typename A, typename B>                                                            \
    __device__ __forceinline__ void name_(acc_t_& acc, const A a0, const A a1, const B b0, const B b1) {                        \
        static_assert(TERMS == 1 || TERMS == 3, "one term or three");                                                            \
        const f16x8 p0 = __builtin_bit_cast(f16x8, a0), q0 = __builtin_bit_cast(f16x8, b0);                                      \
        acc = mfma_(p0, q0, acc, 0, 0, 0);                                                                                       \
        if (TERMS == 3) {                                                                                                        \
            const f16x8 p1 = __builtin_bit_cast(f16x8, a1), q1 = __builtin_bit_cast(f16x8, b1);                                  \
            acc = W_IS_B ? mfma_(p0, q1, acc, 0, 0, 0) : mfma_(p1, q0, acc, 0, 0, 0);                                            \
            acc = W_IS_B ? mfma_(p1, q0, acc, 0, 0, 0) : mfma_(p0, q1, acc, 0, 0, 0);                                            \
        }                                                                                                                        \
    }
FF_MFMA_TERMS(mfma16_terms, f32x4, __builtin_amdgcn_mfma_f32_16x16x32_f16)
FF_MFMA_TERMS(mfma32_terms, f32x16, __builtin_amdgcn_mfma_f32_32x32x16_f16)
#undef FF_MFMA_TERMS

// ---- fragment-order weight image (ff_pack_frag16): [16-channel tile][K chunk][term][lane][16 B] - a wave's load of one term
// is one contiguous KB, the second term 1024 bytes behind the first.  Byte offset = voff (vector) + soff (scalar).
// TERM_IN_SOFF: which of the two the second term's + term_off is added to (an immediate either way, but the kernels' address
// code differs with it).  term_off is 64 when the same loads read packed ROWS instead ([channel][K chunk][term][64 B]).
template <int TERMS, bool TERM_IN_SOFF = false>
__device__ __forceinline__ void load_w_frag(const __amdgpu_buffer_rsrc_t rs, int voff, int soff, f32x4* w, int term_off = 1024) {
    w[0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0));
    if (TERMS == 3)
        w[1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, TERM_IN_SOFF ? voff : voff + term_off, TERM_IN_SOFF ? soff + term_off : soff, 0));
}

}  // namespace ff
