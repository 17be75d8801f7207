// dmr_l2_ref.cpp — the reference's own DMR layer 2 classes behind a C interface, for tests/test_dmr_l2.py and tools/make_dmr_l2_golden.py.
// Includes the reference's headers from where they lie and links oracle/_ref/libqrl_ref.so; nothing of the reference is copied.
//   ref_dmr_l2_record   the 80-byte record of qrl_dmr_l2_decode (include/qrl_hip.h), every byte from the reference's accessors, in the
//                       reference's order: DMRFrame(bytes, type), validate() (src/DMR/dmrcontrol.cpp:630), runAudioFEC() (:233),
//                       CDMREMB::putData (:247)
//   the rest            the reference's encoders, to build inputs, and its bare decoders, to pin the generated code tables
#include <cstdint>
#include <cstring>
#include "src/DMR/dmrframe.h"
#include "src/MMDVM/BPTC19696.h"
#include "src/MMDVM/Golay2087.h"
#include "src/MMDVM/Golay24128.h"
#include "src/MMDVM/QR1676.h"
#include "src/MMDVM/RS129.h"
#include "src/MMDVM/CRC.h"
#include "src/MMDVM/DMRLC.h"

extern "C" {

void ref_dmr_l2_record(const uint8_t* in, int audio_fec, uint8_t* out)
{
    memset(out, 0, 80);
    uint8_t burst[33];
    memcpy(burst, in + 4, 33);
    const uint8_t type = in[0];
    DMRFrame frame(burst, type);
    frame.setFN(in[1]);
    out[0] = frame.getFrameType();
    out[1] = frame.getFN();
    const bool valid = frame.validate();
    const bool voice = type == DMRFrameTypeVoice || type == DMRFrameTypeVoiceSync;
    int errors = 0;
    if (voice && audio_fec) errors = frame.runAudioFEC();
    uint8_t data[33];
    frame.getData(data);
    uint8_t cc = frame.getColorCode();
    if (type == DMRFrameTypeVoiceSync) cc = in[2];
    if (type == DMRFrameTypeVoice) {
        CDMREMB emb;
        emb.putData(data);
        cc = emb.getColorCode();
        out[6] = emb.getPI() ? 1 : 0;
        out[7] = emb.getLCSS();
    }
    out[2] = cc;
    out[3] = frame.getDataType();
    out[4] = valid ? 1 : 0;
    out[5] = (uint8_t)errors;
    out[9] = frame.getFLCO();
    out[10] = frame.getFID();
    const uint32_t src = frame.getSrcId(), dst = frame.getDstId();
    for (int i = 0; i < 4; ++i) { out[12 + i] = (uint8_t)(src >> (8 * i)); out[16 + i] = (uint8_t)(dst >> (8 * i)); }
    memcpy(out + 20, data, 33);
    if (voice) {
        frame.getVoice(out + 53);
        out[8] = 27;
    } else if (type == DMRFrameTypeData && valid) {
        if (frame.getDataType() == DT_RATE_34_DATA) {
            CDMRTrellis trellis;
            trellis.decode(burst, out + 53);
            out[8] = 18;
        } else {
            CBPTC19696 bptc;   // what CDMRCSBK / CDMRDataHeader / CDMRFullLC keep after put(): the decoded block, masks in place
            bptc.decode(burst, out + 53);
            out[8] = 12;
        }
    }
}

int ref_dmr_const(int which)
{
    switch (which) {
    case 0: return DT_VOICE_SYNC;
    case 1: return DT_VOICE;
    case 2: return DMRFrameTypeData;
    case 3: return DMRFrameTypeVoice;
    case 4: return DMRFrameTypeVoiceSync;
    case 5: return DT_RATE_34_DATA;
    case 6: return DT_DATA_HEADER;
    case 7: return DT_CSBK;
    default: return -1;
    }
}

// ---- encoders, to build inputs ----
void ref_trellis_encode(const uint8_t* payload, uint8_t* burst) { CDMRTrellis t; t.encode(payload, burst); }
int ref_trellis_decode(const uint8_t* burst, uint8_t* payload) { CDMRTrellis t; return t.decode(burst, payload) ? 1 : 0; }
void ref_bptc_encode(const uint8_t* payload, uint8_t* burst) { CBPTC19696 b; b.encode(payload, burst); }
void ref_bptc_decode(const uint8_t* burst, uint8_t* payload) { CBPTC19696 b; b.decode(burst, payload); }
void ref_fulllc_encode(const uint8_t* lc9, int type, uint8_t* burst)
{
    CDMRLC lc(lc9);
    CDMRFullLC full;
    full.encode(&lc, burst, (unsigned char)type);
}
void ref_csbk_build(int csbko, int lb, int pf, int fid, int data1, int cbf, uint32_t dst, uint32_t src, int data_type, uint8_t* burst)
{
    CDMRCSBK csbk;
    csbk.setCSBKO((unsigned char)csbko, lb != 0, pf != 0);
    csbk.setFID((unsigned char)fid);
    csbk.setData1((unsigned char)data1);
    csbk.setCBF((unsigned char)cbf);
    csbk.setDstId(dst);
    csbk.setSrcId(src);
    csbk.setDataType((unsigned char)data_type);
    csbk.get(burst);
}
void ref_dataheader_build(const uint8_t* data10, uint8_t* burst)
{
    CDMRDataHeader h;
    uint8_t d[10];
    memcpy(d, data10, 10);
    h.setData(d);
    h.get(burst);
}
void ref_slottype_set(int cc, int dt, uint8_t* burst)
{
    CDMRSlotType st;
    st.setColorCode((unsigned char)cc);
    st.setDataType((unsigned char)dt);
    st.getData(burst);
}
void ref_emb_set(int cc, int pi, int lcss, uint8_t* burst)
{
    CDMREMB emb;
    emb.setColorCode((unsigned char)cc);
    emb.setPI(pi != 0);
    emb.setLCSS((unsigned char)lcss);
    emb.getData(burst);
}
uint32_t ref_golay24128_encode(uint32_t data) { return CGolay24128::encode24128(data); }
uint32_t ref_golay23127_encode(uint32_t data) { return CGolay24128::encode23127(data); }

// ---- bare decoders, to pin the tables ----
int ref_golay2087_decode(const uint8_t* d3) { return CGolay2087::decode(d3); }
int ref_qr1676_decode(const uint8_t* d2) { return CQR1676::decode(d2); }
uint32_t ref_golay23127_decode(uint32_t code) { return CGolay24128::decode23127(code); }
int ref_golay24128_decode(uint32_t code, uint32_t* data) { unsigned int o = 0; const bool v = CGolay24128::decode24128(code, o); *data = o; return v ? 1 : 0; }
int ref_rs129_check(const uint8_t* d12) { return CRS129::check(d12) ? 1 : 0; }
int ref_crc_ccitt162_check(const uint8_t* d12) { return CCRC::checkCCITT162(d12, 12U) ? 1 : 0; }
unsigned ref_ambe_regenerate(uint8_t* burst) { CAMBEFEC fec; return fec.regenerateDMR(burst); }

}
