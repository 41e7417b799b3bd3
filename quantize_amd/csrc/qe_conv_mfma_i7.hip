// qe_conv_mfma_i7.hip -- instantiations of the flat 1x1 kernel for small planes (several whole images per tile).
#include "qe_conv_mfma_kernel.hpp"

namespace qe {

template <int NS>
static MfmaLaunch flatg_w(bool wraw)   // 49-pixel planes
{
    return wraw ? &mfma_launch<&conv_mfma_flatg_kernel<7, NS, true, 7>> : &mfma_launch<&conv_mfma_flatg_kernel<7, NS, false, 7>>;
}

MfmaLaunch mfma_flatg(int niw, int ns, bool wraw)
{
    if (niw != 7) return nullptr;
    switch (ns) {
        case 4: return flatg_w<4>(wraw);
        case 2: return flatg_w<2>(wraw);
    }
    return nullptr;
}

}  // namespace qe
