// The int8 work() overload of the transmitter facade (qradiolink_amd/host/gr_modem_hip.*) against the C ABI call it wraps:
//   test_sc8_tx_work <modem_type> <other_modem_type> <streams> <rate> <offset_hz> <bb_gain> <sc8_scale> <nbytes> <bytes.bin> <out_prefix>
//     bytes.bin = streams x nbytes bytes (stream-major).
//     facade: a gr_mod_base_hip at <rate> gets set_sc8_scale(<sc8_scale>) BEFORE any mode is open, then set_mode(<other>), set_mode(<modem>): the scale
//             has to survive both.  Its queue is drained through work(int8_t* const*)  ->  <out_prefix>.facade.<s>.bin (interleaved int8 I, Q);
//             clipped(s) is printed as clipped.<s>=N.
//     C ABI:  qrl_mod_create with the same settings, qrl_mod_set_sc8_scale, qrl_mod_set_sc8_clip_counts, one qrl_mod_process_sc8 of all the bytes
//             ->  <out_prefix>.abi.<s>.bin, abi_clipped.<s>=N.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "gr_modem_hip.h"

using namespace qrl_host;

static void dump(const std::string& name, const std::vector<int8_t>& v)
{
    std::ofstream o(name, std::ios::binary);
    o.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)v.size());
}
static void must(bool ok, const char* what) { if (!ok) throw std::runtime_error(what); }

static int run(char** argv)
{
    const int mode = atoi(argv[1]), other = atoi(argv[2]), S = atoi(argv[3]), rate = atoi(argv[4]);
    const double offset = atof(argv[5]);
    const float gain = (float)atof(argv[6]), scale = (float)atof(argv[7]);
    const size_t n = (size_t)atoll(argv[8]);
    std::vector<uint8_t> bytes((size_t)S * n);
    {
        std::ifstream f(argv[9], std::ios::binary);
        f.read(reinterpret_cast<char*>(bytes.data()), (std::streamsize)bytes.size());
        must((bool)f, "short input");
    }
    const std::string prefix = argv[10];
    qrl_runtime rt(0);
    {
        gr_mod_base_hip mod(rt, S, rate, offset, n);
        mod.set_sc8_scale(scale);
        mod.set_mode(other);
        mod.set_mode(mode);
        mod.set_bb_gain(gain);
        for (int s = 0; s < S; ++s) mod.set_data(new std::vector<uint8_t>(bytes.begin() + (size_t)s * n, bytes.begin() + (size_t)(s + 1) * n), s);
        const size_t cap = mod.samples_per_byte() * n;
        std::vector<std::vector<int8_t>> buf((size_t)S, std::vector<int8_t>(2 * cap)), got((size_t)S);
        std::vector<int8_t*> p((size_t)S);
        for (int s = 0; s < S; ++s) p[(size_t)s] = buf[(size_t)s].data();
        for (;;) {
            const size_t ns = mod.work(p.data());
            if (!ns) break;
            for (int s = 0; s < S; ++s) got[(size_t)s].insert(got[(size_t)s].end(), buf[(size_t)s].begin(), buf[(size_t)s].begin() + 2 * ns);
        }
        for (int s = 0; s < S; ++s) {
            dump(prefix + ".facade." + std::to_string(s) + ".bin", got[(size_t)s]);
            std::cout << "clipped." << s << "=" << mod.clipped(s) << "\n";
        }
    }
    {
        qrl_mod_config c{};
        c.modem_type = mode; c.use_mode_defaults = 1; c.batch = S; c.max_bytes = n; c.bb_gain = gain; c.device_samp_rate = rate; c.carrier_offset_hz = offset;
        qrl_mod* h = nullptr;
        must(qrl_mod_create(rt.ctx(), &c, &h) == QRL_OK, "qrl_mod_create");
        const size_t count = qrl_mod_samples_per_byte(h) * n;
        uint8_t* d_bytes = nullptr; int8_t* d_iq = nullptr; uint32_t* d_clip = nullptr;
        must(hipMalloc((void**)&d_bytes, bytes.size()) == hipSuccess && hipMalloc((void**)&d_iq, 2 * count * (size_t)S) == hipSuccess &&
             hipMalloc((void**)&d_clip, sizeof(uint32_t) * (size_t)S) == hipSuccess, "hipMalloc");
        must(hipMemcpy(d_bytes, bytes.data(), bytes.size(), hipMemcpyHostToDevice) == hipSuccess && hipMemset(d_clip, 0, sizeof(uint32_t) * (size_t)S) == hipSuccess &&
             hipDeviceSynchronize() == hipSuccess, "upload");
        must(qrl_mod_set_sc8_scale(h, scale) == QRL_OK && qrl_mod_set_sc8_clip_counts(h, d_clip) == QRL_OK, "sc8 setters");
        must(qrl_mod_process_sc8(h, d_bytes, n, n, d_iq, count) == QRL_OK && qrl_mod_sync(h) == QRL_OK, "qrl_mod_process_sc8");
        std::vector<int8_t> row(2 * count);
        std::vector<uint32_t> clip((size_t)S);
        must(hipMemcpy(clip.data(), d_clip, sizeof(uint32_t) * (size_t)S, hipMemcpyDeviceToHost) == hipSuccess, "D2H");
        for (int s = 0; s < S; ++s) {
            must(hipMemcpy(row.data(), d_iq + 2 * count * (size_t)s, 2 * count, hipMemcpyDeviceToHost) == hipSuccess, "D2H");
            dump(prefix + ".abi." + std::to_string(s) + ".bin", row);
            std::cout << "abi_clipped." << s << "=" << clip[(size_t)s] << "\n";
        }
        qrl_mod_destroy(h);
        (void)hipFree(d_bytes); (void)hipFree(d_iq); (void)hipFree(d_clip);
    }
    return 0;
}

int main(int argc, char** argv)
{
    try {
        if (argc == 11) return run(argv);
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << "\n";
        return 1;
    }
    std::cerr << "usage: test_sc8_tx_work <modem> <other_modem> <streams> <rate> <offset_hz> <bb_gain> <sc8_scale> <nbytes> <bytes.bin> <out_prefix>\n";
    return 2;
}
