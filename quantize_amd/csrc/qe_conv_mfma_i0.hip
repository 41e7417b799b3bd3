// qe_conv_mfma_i0.hip -- instantiations of conv_mfma_kernel for the 4x1 wave layout.
#include "qe_conv_mfma_kernel.hpp"

namespace qe {

MfmaLaunch mfma_halo_cfg0(int niw, int kkt, int ns, bool rq, bool patch)
{
    switch (niw) {
        case 7: return mfma_halo<4, 1, 7>(kkt, ns, rq, patch);
        case 4: return mfma_halo<4, 1, 4>(kkt, ns, rq, patch);
        case 2: return mfma_halo<4, 1, 2>(kkt, ns, rq, patch);
    }
    return nullptr;
}

}  // namespace qe
