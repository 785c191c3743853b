// SDP passes (c4_sdp_wave.h) of the coding2genome family (boundary flavour, query advance up to 3): reverse and forward sweep
#include "../c4_sdp_launch.h"
namespace c4sdp {
C4SDP_DEFINE_KERNELS(sdp_kernels_coding2genome, c4k::Coding2GenomeDesc, true)
}
