// jump_host.cpp -- the product's host jump-ahead (csrc/gf2.hpp) as a stand-alone program, for tests/test_jump_host.py.
//
//   jump_host apply|power <matrix.taps | prbs:K> <init hex> < positions
//
// reads decimal stream positions N from standard input, one per line, and prints A^N init as hex, one per line.
// `apply` is GF2Powers::apply (what bbb_lutopt_state_at and bbb_prbs_state_at call), `power` is GF2Powers::power followed
// by one matrix-vector product (what builds B = A^L for the device seeding).  The test compiles this file against a COPY
// of gf2.hpp: once as it is, and once per mutant with one jump error put in by exact text.
#include "gf2.hpp"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

int main(int argc, char **argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: jump_host apply|power <matrix.taps | prbs:K> <init hex>\n"); return 2; }
    const std::string via = argv[1], what = argv[2];
    std::string hex = argv[3];
    if (via != "apply" && via != "power") { std::fprintf(stderr, "unknown route %s\n", via.c_str()); return 2; }
    bbb::GF2Mat A;
    if (what.rfind("prbs:", 0) == 0) {
        const int k = std::atoi(what.c_str() + 5);
        if (!bbb::prbs_tap(k)) { std::fprintf(stderr, "k=%d invalid for PRBS\n", k); return 2; }
        A = bbb::prbs_matrix(k, bbb::prbs_tap(k));
    } else {
        std::ifstream f(what);
        std::vector<std::vector<int>> rows;
        for (std::string line; std::getline(f, line);) {
            std::istringstream ls(line);
            std::vector<int> r;
            for (int c; ls >> c;) r.push_back(c);
            if (!r.empty()) rows.push_back(r);
        }
        const int k = (int)rows.size();
        if (k < 1 || k > 512) { std::fprintf(stderr, "cannot read %s\n", what.c_str()); return 2; }
        A = bbb::GF2Mat(k);
        for (int r = 0; r < k; r++)
            for (int c : rows[(size_t)r]) {
                if (c < 0 || c >= k) { std::fprintf(stderr, "tap out of range\n"); return 2; }
                A.set(r, c);
            }
    }
    if (hex.size() > 128) { std::fprintf(stderr, "init too wide\n"); return 2; }
    uint64_t x0[8] = {0};
    for (size_t i = 0; i < hex.size(); i++) {
        const char ch = hex[hex.size() - 1 - i];
        const int v = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : ch >= 'A' && ch <= 'F' ? ch - 'A' + 10 : -1;
        if (v < 0 || (int)(4 * i) >= 64 * A.W) { std::fprintf(stderr, "bad init\n"); return 2; }
        x0[i / 16] |= (uint64_t)v << (4 * (i % 16));
    }
    bbb::GF2Powers pw(A);
    for (std::string line; std::getline(std::cin, line);) {
        if (line.empty()) continue;
        const uint64_t n = std::strtoull(line.c_str(), nullptr, 10);
        uint64_t y[8] = {0};
        if (via == "apply")
            pw.apply(n, x0, y);
        else
            pw.power(n).matvec(x0, y);
        for (int w = A.W - 1; w >= 0; w--) std::printf("%016llx", (unsigned long long)y[w]);
        std::printf("\n");
    }
    return 0;
}
