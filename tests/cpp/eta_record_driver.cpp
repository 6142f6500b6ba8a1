// The host half of imported eta records (hydrochrono_amd/csrc/hc_eta_record.hpp) without a GPU: the reference's file format, the
// record validation and the zero extension.  Built with plain g++ by tests/test_eta_record_cpu.py.
//   usage: eta_record_driver parse    <file>                      "n <n>", "first <t> <eta>", "last <t> <eta>"  (or "error <message>")
//          eta_record_driver validate <file>                      "ok"                                          (or "error <message>")
//          eta_record_driver extend   <file> <tau_min> <tau_max>  "h <h>", "front <n>", "back <n>", "size <n>", "t <first> <last>",
//                                                                 "record <t at n_front> <t at n_front + n - 1>", then "<t> <eta>" per sample
// Numbers are printed with %.17g.  Exit 0 on success, 1 on an error line.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../hydrochrono_amd/csrc/hc_eta_record.hpp"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string mode = argv[1], path = argv[2];
    std::vector<double> t, eta;
    std::string err = hc::read_eta_file(path, t, eta);
    if (err.empty() && mode != "parse") err = hc::validate_eta_record(t.data(), eta.data(), static_cast<long long>(t.size()));
    if (!err.empty()) {
        std::printf("error %s\n", err.c_str());
        return 1;
    }
    if (mode == "parse") {
        std::printf("n %zu\n", t.size());
        if (!t.empty()) {
            std::printf("first %.17g %.17g\n", t.front(), eta.front());
            std::printf("last %.17g %.17g\n", t.back(), eta.back());
        }
        return 0;
    }
    if (mode == "validate") {
        std::printf("ok\n");
        return 0;
    }
    if (mode == "extend" && argc >= 5) {
        const long long n        = static_cast<long long>(t.size());
        const hc::EtaExtended x = hc::extend_eta_record(t.data(), eta.data(), n, std::atof(argv[3]), std::atof(argv[4]));
        std::printf("h %.17g\nfront %lld\nback %lld\nsize %zu\n", x.h, x.n_front, x.n_back, x.t.size());
        std::printf("t %.17g %.17g\n", x.t.front(), x.t.back());
        std::printf("record %.17g %.17g\n", x.t[x.n_front], x.t[x.n_front + n - 1]);
        for (size_t i = 0; i < x.t.size(); ++i) std::printf("%.17g %.17g\n", x.t[i], x.eta[i]);
        return 0;
    }
    return 2;
}
