// qe_conv_mfma_i6.hip -- instantiations of the two-strips-per-wave 3x3 MFMA kernel.
#include "qe_conv_mfma_kernel.hpp"

namespace qe {

// every re-quantising instance has its PATCH form; up to 80 KB of dynamic LDS
template <int WMS, int SPLIT>
static MfmaLaunch sm2_rq(bool rq, bool patch)
{
    if (!rq) return patch ? nullptr : &mfma_launch<&conv_mfma_sm2_kernel<WMS, 9, SPLIT, false, false>, MF_THREADS, MF_MAX_LDS_SM2>;
    if (!patch) return &mfma_launch<&conv_mfma_sm2_kernel<WMS, 9, SPLIT, true, false>, MF_THREADS, MF_MAX_LDS_SM2>;
    return &mfma_launch<&conv_mfma_sm2_kernel<WMS, 9, SPLIT, true, true>, MF_THREADS, MF_MAX_LDS_SM2>;
}
template <int WMS>
static MfmaLaunch sm2_split(int split, bool rq, bool patch)
{
    switch (split) {
        case 4: return sm2_rq<WMS, 4>(rq, patch);
        case 2: return sm2_rq<WMS, 2>(rq, patch);
        case 1: return sm2_rq<WMS, 1>(rq, patch);
    }
    return nullptr;
}

MfmaLaunch mfma_sm2(int wms, int split, bool rq, bool patch)
{
    switch (wms) {
        case 2: return sm2_split<2>(split, rq, patch);
        case 1: return sm2_split<1>(split, rq, patch);
    }
    return nullptr;
}

}  // namespace qe
