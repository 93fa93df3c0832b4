// Driver of tests/test_kmer_plan.py: carpedeam_amd/csrc/kmer_plan.h alone (it must compile without HIP), asked line by line on stdin.
//   L entry n maxLen residues k deviceBytes layout forceHuge forceWideKey kmerSort kmerPasses overRanks   -> the layout's name
//   C parts bins h[0] .. h[bins - 1]                                                                       -> the cuts
//   P n residues deviceBytes valBytes                                                                      -> P B
#include <cstdio>
#include <iostream>
#include <string>
#include "../../carpedeam_amd/csrc/kmer_plan.h"

int main() {
    using namespace kplan;
    static const char *names[] = {"Slot", "Packed", "Wide", "Long", "Huge", "TooLong", "BadSwitch", "PackedUnfit", "SlotUnfit"};
    std::ios::sync_with_stdio(false);
    std::string cmd, out;
    while (std::cin >> cmd) {
        if (cmd == "L") {
            int entry, layout, fh, fw, ks, kp, ranks; Db d; Switches sw;
            std::cin >> entry >> d.n >> d.maxLen >> d.residues >> d.k >> d.deviceBytes >> layout >> fh >> fw >> ks >> kp >> ranks;
            sw.layout = (LayoutSwitch) layout; sw.forceHuge = fh; sw.forceWideKey = fw; sw.kmerSort = ks; sw.kmerPasses = kp;
            out += names[(int) chooseLayout((Entry) entry, d, sw, ranks != 0)];
        } else if (cmd == "C") {
            int parts, bins; std::cin >> parts >> bins;
            std::vector<unsigned long long> h((size_t) bins);
            for (auto &x : h) std::cin >> x;
            for (uint32_t c : equalShareCuts(h.data(), bins, parts)) out += std::to_string(c) + " ";
        } else if (cmd == "P") {
            Db d; size_t valBytes; std::cin >> d.n >> d.residues >> d.deviceBytes >> valBytes;
            const PassPlan pl = passPlan(d, valBytes);
            out += std::to_string(pl.P) + " " + std::to_string(pl.B);
        } else return 2;
        out += "\n";
    }
    fputs(out.c_str(), stdout);
    return 0;
}
