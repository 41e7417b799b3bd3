// qe_conv_mfma_i3.hip -- instantiations of the small-IC (stem) MFMA kernel.
#include "qe_conv_mfma_kernel.hpp"

namespace qe {

// PATCH form: the instances with 7 column tiles per wave
template <int WM, int WN, int NIW>
static MfmaLaunch stem_rq(bool rq, bool patch)
{
    if (!rq) return patch ? nullptr : &mfma_launch<&conv_mfma_smallic_kernel<WM, WN, NIW, false>>;
    if (!patch) return &mfma_launch<&conv_mfma_smallic_kernel<WM, WN, NIW, true>>;
    if constexpr (NIW == 7) return &mfma_launch<&conv_mfma_smallic_kernel<WM, WN, NIW, true, true>>;
    return nullptr;
}

MfmaLaunch mfma_stem(int cfg, int niw, bool rq, bool patch)
{
    switch (cfg) {
        case 0: return niw == 7 ? stem_rq<4, 1, 7>(rq, patch) : nullptr;
        case 1: return niw == 7 ? stem_rq<2, 2, 7>(rq, patch) : nullptr;   // 64 output channels, 448-pixel tiles (4 rows of the 112-wide stem output)
        case 2: return niw == 2 ? stem_rq<1, 4, 2>(rq, patch) : nullptr;
    }
    return nullptr;
}

}  // namespace qe
