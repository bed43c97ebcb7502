// rip_raw16.hip -- bayer_*16 frames with a 16-bit range (rip_set_debayer_16bit + rip_set_debayer_16bit_range): demosaic at 16 bits,
// narrowing to 8 bits and the flip of flip.cpp:40-52 in ONE pass, 2 B/px read, 3 B/px written.  Everything behind it sees the
// result exactly as it would see a bgr8 frame holding it (PARITY.md "16-bit Bayer frames through the whole chain").
//
// Contract:
//   demosaic   bilinear: the two-tap / four-tap rounding averages of debayer16_kernel (rip_chain.hip; cv::demosaicing's
//              Bayer2RGB_Invoker<ushort>), border rule: the interior formula at the position clamped to [1, n - 2].
//              mht: the four 5 x 5 filters of rip_demosaic.hip on 16-bit samples, rounded half to even, clamped to [0, 65535],
//              reflect-101 reads outside the frame.
//   narrowing  n(v) = min(255, floor((510 * max(v - black, 0) + R) / (2 R))), R = white - black: 255 (v - black) / R rounded half
//              up.  No division in the loop: t = clamp(v - black, 0, R) makes the numerator 510 t + R < 2^26, and for numerators
//              below 2^N the quotient by d is (num * M) >> (N + l) with l = ceil(log2 d), M = ceil(2^(N + l) / d) (Granlund and
//              Montgomery, "Division by invariant integers using multiplication", PLDI 1994, theorem 4.2).  N = 26, d = 2 R:
//              2^26 <= M < 2^27; the numerator is shifted left by 6 so that the quotient is v_mul_hi_u32's result shifted right
//              by l.  The clamp to R also stands in for MHT's clamp to [0, 65535] (black >= 0, black + R <= 65535).
//
// The kernel is raw16_tile_kernel of rip_raw16_dev.hpp, which the packed 10- / 12-bit formats share (rip_packed.hip): here with
// the uint16 staging, 2 B/px read.  Its description is there.
#include "rip_raw16_dev.hpp"

namespace rip {

void raw16_narrow_constants(int black, int white, uint32_t* mul, int* shift) {
  const unsigned long long d = 2ull * (unsigned long long)(white - black);
  int l = 0;
  while ((1ull << l) < d) l++;
  *mul = (uint32_t)(((1ull << (26 + l)) + d - 1) / d);
  *shift = l;
}

void launch_raw16(const Raw16Params& p, hipStream_t stream) { launch_tiles<StageU16>(p, stream); }

}  // namespace rip
