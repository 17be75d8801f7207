// dmr_alias_ref.cpp — the reference's DMRUtils::parseISO7bitToISO8bit behind a C interface, for tests/test_dmr_rx.py: compiled together with the
// reference's src/DMR/dmrutils.cpp, unmodified, against the QString / QSysInfo stand-ins of tests/host/dmr_ctl_stub; nothing of the reference is copied.
#include <cstring>
#include <vector>
#include "src/DMR/dmrutils.h"

extern "C" int ref_alias_7bit(const unsigned char* msg, unsigned size, unsigned char* out)
{
    const unsigned bit7_size = 8 * size / 7;
    std::vector<unsigned char> in(msg, msg + size), conv(bit7_size + 2, 0);   // one more than the reference's own buffer: its last step may write there
    DMRUtils::parseISO7bitToISO8bit(in.data(), conv.data(), bit7_size, size);
    memcpy(out, conv.data(), bit7_size);
    return (int)bit7_size;
}
