// qe_conv_mfma_i2.hip -- instantiations of conv_mfma_kernel for the 1x4 wave layout.
#include "qe_conv_mfma_kernel.hpp"

namespace qe {

MfmaLaunch mfma_halo_cfg2(int niw, int kkt, int ns, bool rq, bool patch)
{
    switch (niw) {
        case 2: return mfma_halo<1, 4, 2>(kkt, ns, rq, patch);
        case 1: return mfma_halo<1, 4, 1>(kkt, ns, rq, patch);
    }
    return nullptr;
}

}  // namespace qe
