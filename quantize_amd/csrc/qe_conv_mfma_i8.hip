// qe_conv_mfma_i8.hip -- instantiations of the flat 1x1 MFMA kernel for 4-bit activations read from the packed stream
// (128-channel workgroups, prepared weight fragments).
#include "qe_conv_mfma_kernel.hpp"

namespace qe {

template <int NIW>
static MfmaLaunch flat4_ns(int ns)
{
    switch (ns) {
        case 4: return &mfma_launch<&conv_mfma_flat_kernel<4, 1, NIW, 4, false, false, true>>;
        case 2: return &mfma_launch<&conv_mfma_flat_kernel<4, 1, NIW, 2, false, false, true>>;
        case 1: return &mfma_launch<&conv_mfma_flat_kernel<4, 1, NIW, 1, false, false, true>>;
    }
    return nullptr;
}

MfmaLaunch mfma_flat_x4(int niw, int ns)
{
    switch (niw) {
        case 4: return flat4_ns<4>(ns);
        case 5: return flat4_ns<5>(ns);
        case 7: return flat4_ns<7>(ns);
    }
    return nullptr;
}

}  // namespace qe
