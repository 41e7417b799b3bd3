// qe_conv_mfma_i1.hip -- instantiations of conv_mfma_kernel for the 2x2 wave layout.
#include "qe_conv_mfma_kernel.hpp"

namespace qe {

MfmaLaunch mfma_halo_cfg1(int niw, int kkt, int ns, bool rq, bool patch)
{
    switch (niw) {
        case 4: return mfma_halo<2, 2, 4>(kkt, ns, rq, patch);
        case 2: return mfma_halo<2, 2, 2>(kkt, ns, rq, patch);
        case 1: return mfma_halo<2, 2, 1>(kkt, ns, rq, patch);
    }
    return nullptr;
}

}  // namespace qe
