// rip_packed.hip -- packed 10- / 12-bit Bayer frames (bayer_*10p, *12p, *10_csi2, *12_csi2; rip.h "Packed Bayer frames"): the
// kernel of rip_raw16.hip with the packed stagings of rip_raw16_dev.hpp -- the bytes are unpacked on their way into the LDS tile,
// 1.25 or 1.5 B/px read, and the demosaic, the narrowing with the effective range, the flip and the stores are the shared code.
#include "rip_raw16_dev.hpp"

namespace rip {

void launch_packed(const Raw16Params& p, int layout, hipStream_t stream) {
  switch (layout) {
    case PACKED_10P: launch_tiles<StagePacked<PACKED_10P>>(p, stream); break;
    case PACKED_12P: launch_tiles<StagePacked<PACKED_12P>>(p, stream); break;
    case PACKED_10_CSI2: launch_tiles<StagePacked<PACKED_10_CSI2>>(p, stream); break;
    default: launch_tiles<StagePacked<PACKED_12_CSI2>>(p, stream); break;
  }
}

}  // namespace rip
