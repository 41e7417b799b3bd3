// qe_conv_mfma_i4.hip -- instantiations of the flat 1x1 MFMA kernel.
#include "qe_conv_mfma_kernel.hpp"

namespace qe {

template <int WM, int WN, int NIW, bool WRAW>
static MfmaLaunch flat_ns(int ns)
{
    switch (ns) {
        case 4: return &mfma_launch<&conv_mfma_flat_kernel<WM, WN, NIW, 4, WRAW, false>>;
        case 2: return &mfma_launch<&conv_mfma_flat_kernel<WM, WN, NIW, 2, WRAW, false>>;
        case 1: return &mfma_launch<&conv_mfma_flat_kernel<WM, WN, NIW, 1, WRAW, false>>;
    }
    return nullptr;
}
template <int WM, int WN, int NIW>
static MfmaLaunch flat_w(int ns, bool wraw)
{
    return wraw ? flat_ns<WM, WN, NIW, true>(ns) : flat_ns<WM, WN, NIW, false>(ns);
}

MfmaLaunch mfma_flat(int cfg, int niw, int ns, bool wraw, bool s2)
{
    if (s2) {   // stride-2 1x1: 224-pixel tiles, 64-channel stages, 128-channel workgroups only
        if (cfg != 0 || niw != 7 || ns != 2) return nullptr;
        return wraw ? &mfma_launch<&conv_mfma_flat_kernel<4, 1, 7, 2, true, true>> : &mfma_launch<&conv_mfma_flat_kernel<4, 1, 7, 2, false, true>>;
    }
    switch (cfg) {
        case 0:
            switch (niw) {
                case 4: return flat_w<4, 1, 4>(ns, wraw);
                case 5: return flat_w<4, 1, 5>(ns, wraw);
                case 7: return flat_w<4, 1, 7>(ns, wraw);
            }
            return nullptr;
        case 1: return niw == 4 ? flat_w<2, 2, 4>(ns, wraw) : nullptr;
        case 2: return niw == 2 ? flat_w<1, 4, 2>(ns, wraw) : nullptr;
    }
    return nullptr;
}

}  // namespace qe
