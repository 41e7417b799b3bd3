// qe_conv_mfma_i5.hip -- instantiations of the warp-specialised 3x3 MFMA kernel.
#include "qe_conv_mfma_kernel.hpp"

namespace qe {

template <int NIW, int SPLIT>
static MfmaLaunch ws_rq(bool rq)
{
    return rq ? &mfma_launch<&conv_mfma_ws_kernel<NIW, 9, SPLIT, true>, 2 * MF_THREADS>
              : &mfma_launch<&conv_mfma_ws_kernel<NIW, 9, SPLIT, false>, 2 * MF_THREADS>;
}
template <int NIW>
static MfmaLaunch ws_split(int split, bool rq)
{
    switch (split) {
        case 4: return ws_rq<NIW, 4>(rq);
        case 2: return ws_rq<NIW, 2>(rq);
        case 1: return ws_rq<NIW, 1>(rq);
    }
    return nullptr;
}

MfmaLaunch mfma_ws(int niw, int split, bool rq)
{
    switch (niw) {
        case 7: return ws_split<7>(split, rq);
        case 4: return ws_split<4>(split, rq);
        case 2: return ws_split<2>(split, rq);
    }
    return nullptr;
}

}  // namespace qe
