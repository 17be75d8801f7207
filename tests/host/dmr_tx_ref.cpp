// dmr_tx_ref.cpp — the reference's own DMR transmit frame layer behind a C interface, for tests/test_dmr_tx.py and
// tools/make_dmr_tx_golden.py.  Includes the reference's headers from where they lie, links oracle/_ref/libqrl_ref.so and is compiled
// together with the reference's src/DMR/dmrcontrol.cpp, unmodified, against the stand-ins of tests/host/dmr_ctl_stub; nothing of the
// reference is copied.
//   ref_dmr_tx_record   one 48-byte TX record (include/qrl_hip.h) -> the 33 bytes DMRFrame holds after the reference's own calls per kind
//   ref_dmr_tx_call     a whole call through DMRControl: getStartCSBK, getVoiceHeader, initVoiceTX, addTxAudio / getTxAudio per voice
//                       burst, stopVoiceTX, the terminator, and the frames gr_modem::transmitDMR adds behind it (src/gr_modem.cpp:786-800)
#include <cstdint>
#include <cstring>
#include <vector>
#include "src/DMR/dmrcontrol.h"
#include "src/DMR/dmrframe.h"
#include "src/MMDVM/BPTC19696.h"
#include "src/MMDVM/CRC.h"
#include "src/MMDVM/DMRLC.h"
#include "src/MMDVM/Sync.h"

// the signals of DMRControl, which moc would write: nobody listens
void DMRControl::digitalAudio(unsigned char* audiodata, int) { delete[] audiodata; }
void DMRControl::talkerAlias(QString, bool) {}
void DMRControl::gpsInfo(QString, bool) {}
void DMRControl::headerReceived(QString, bool) {}
void DMRControl::terminatorReceived(QString, bool) {}
void DMRControl::endBeep() {}

// a burst CDMRCSBK::put / CDMRDataHeader::put accepts for the ten bytes: their CRC under the mask, BPTC
static void checked_block(const uint8_t* data10, const uint8_t* mask, uint8_t* burst)
{
    uint8_t d[12] = {};
    memcpy(d, data10, 10);
    CCRC::addCCITT162(d, 12U);
    d[10] ^= mask[0]; d[11] ^= mask[1];
    CBPTC19696 bptc;
    bptc.encode(d, burst);
}
static void slot_type_and_sync(uint8_t cc, uint8_t dt, uint8_t* burst)
{
    CDMRSlotType st;
    st.setColorCode(cc);
    st.setDataType(dt);
    st.getData(burst);
    CSync::addDMRDataSync(burst, false);
}

extern "C" {

void ref_dmr_tx_record(const uint8_t* rec, uint8_t* burst)
{
    memset(burst, 0, 33);
    const uint8_t kind = rec[0], fn = rec[1], cc = rec[2], dt = rec[3];
    uint8_t pay[27];
    memcpy(pay, rec + 16, 27);
    uint8_t tmp[33] = {};
    switch (kind) {
    case 0: {   // gr_modem.cpp:793-796
        DMRFrame frame(DMRFrameTypeData);
        frame.setSlotNo(0);
        frame.getData(burst);
        break;
    }
    case 1: {
        if (dt != DT_VOICE_LC_HEADER && dt != DT_TERMINATOR_WITH_LC) break;   // CDMRFullLC::encode writes nothing: the reference's bytes are undefined
        CDMRLC lc(rec + 4);
        DMRFrame frame(DMRFrameTypeData);
        frame.setDataType(dt);
        frame.setColorCode(cc);
        frame.constructLCFrame(&lc);
        frame.getData(burst);
        break;
    }
    case 2: {
        checked_block(pay, CSBK_CRC_MASK, tmp);
        CDMRCSBK csbk;
        if (!csbk.put(tmp)) break;
        DMRFrame frame(DMRFrameTypeData);
        frame.setDataType(dt);
        frame.setColorCode(cc);
        frame.constructCSBKFrame(csbk);
        frame.getData(burst);
        break;
    }
    case 3: {
        checked_block(pay, DATA_HEADER_CRC_MASK, tmp);
        CDMRDataHeader header;
        if (!header.put(tmp)) break;
        header.get(burst);
        slot_type_and_sync(cc, dt, burst);
        break;
    }
    case 4: {
        CBPTC19696 bptc;
        bptc.encode(pay, burst);
        slot_type_and_sync(cc, dt, burst);
        break;
    }
    case 5: {
        CDMRTrellis trellis;
        trellis.encode(pay, burst);
        slot_type_and_sync(cc, dt, burst);
        break;
    }
    case 7: {
        DMRFrame frame(DMRFrameTypeVoiceSync);
        frame.setColorCode(cc);
        frame.setVoice(pay);
        frame.addVoiceSync();
        frame.getData(burst);
        break;
    }
    case 8: {
        CDMRLC lc(rec + 4);
        CDMREmbeddedData emb;
        emb.setLC(lc);
        DMRFrame frame(DMRFrameTypeVoice);
        frame.setColorCode(cc);
        frame.setVoice(pay);
        frame.setEmbeddedData(emb, fn);
        frame.getData(burst);
        break;
    }
    default: break;
    }
}

// call: the 40-byte descriptor of qrl_dmr_voice_call_encode (FLCO 0 or 3, FID 0 or 0xC2: what Settings can say); voice [n_voice][27];
// out [3 * repeater + 2 + n_voice + 4][33].  Returns the number of frames written.  The reference ends a call only at a superframe
// boundary: behind stopVoiceTX it goes on sending voice until FN is back at 0, so codec frames of zeros are fed until the terminator
// comes; those extra voice bursts are not written, *extra counts them.
int ref_dmr_tx_call(const uint8_t* call, int repeater, int n_voice, const uint8_t* voice, uint8_t* out, int* extra)
{
    Settings settings;
    Logger logger;
    settings.dmr_source_id = (uint32_t)call[0] << 16 | (uint32_t)call[1] << 8 | call[2];
    settings.dmr_destination_id = (uint32_t)call[3] << 16 | (uint32_t)call[4] << 8 | call[5];
    settings.dmr_call_type = call[6] == FLCO_GROUP ? DMR_CALL_TYPE::GROUP_CALL : DMR_CALL_TYPE::PRIVATE_CALL;
    settings.dmr_vocoder = call[7] == 0xC2 ? 0 : 1;
    settings.dmr_color_code = call[8];
    settings.dmr_timeslot = 1;
    settings.dmr_mode = repeater ? DMR_MODE::DMR_MODE_REPEATER : DMR_MODE::DMR_MODE_DMO;
    settings.dmr_talker_alias = QString(std::string((const char*)call + 9, 27));
    DMRControl control(&settings, &logger);
    std::vector<DMRFrame> frames;
    int n = 0;
    auto put = [&](const DMRFrame& f) { f.getData(out + 33 * n++); };
    if (repeater) { control.getStartCSBK(frames); for (auto& f : frames) put(f); frames.clear(); }   // gr_modem.cpp:676-678
    control.getVoiceHeader(frames);                                                                  // :759-762
    for (auto& f : frames) put(f);
    frames.clear();
    control.initVoiceTX();
    auto feed = [&](const uint8_t* v27) {
        for (int k = 0; k < 3; ++k) {
            unsigned char* a = new unsigned char[9];
            if (v27) memcpy(a, v27 + 9 * k, 9); else memset(a, 0, 9);
            control.addTxAudio(a);
        }
    };
    for (int i = 0; i < n_voice; ++i) {
        feed(voice + 27 * i);
        DMRFrame frame(DMRFrameTypeVoice);
        frame.setDataType(DT_VOICE);
        if (!control.getTxAudio(frame)) return -1;
        put(frame);
    }
    control.stopVoiceTX();
    *extra = 0;
    for (;;) {
        feed(nullptr);
        DMRFrame frame(DMRFrameTypeVoice);
        frame.setDataType(DT_VOICE);
        if (!control.getTxAudio(frame)) return -1;
        if (frame.getDataType() == DT_TERMINATOR_WITH_LC) {   // :790-797
            put(frame); put(frame);
            DMRFrame frame_end(DMRFrameTypeData);
            frame_end.setSlotNo(0);
            put(frame_end); put(frame_end);
            break;
        }
        if (++*extra > 6) return -1;
    }
    return n;
}

}
