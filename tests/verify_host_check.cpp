// CPU check of the verifier's host maths (plonky3_eon_amd/host/verify_host.h), compiled stand-alone
// with the host compiler.  Reads one case per line from the file named on the command line and
// prints one result line each; values are canonical integers as 64 hex digits (the program converts
// to and from the Montgomery form the header works in).  tests/test_verify_host.py writes the cases
// and compares every line with oracle/verify_oracle.py and big integers.
//   inv a                      -> inv <a^-1>            (a != 0)
//   add a b | sub a b          -> add|sub <a +- b>
//   sel log_n zeta             -> sel 1 <first> <last> <transition> <inv_vanishing> | sel 0
//   rec log_n log_qd zeta c... -> rec <quotient(zeta)>  (2^log_qd chunk values)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "verify_host.h"

using namespace eon_host;

static Fr parse(const std::string& s) {  // 64 hex digits, big-endian, canonical -> Montgomery
    Fr v = Fr::zero();
    for (int i = 0; i < 4; i++) v.l[3 - i] = strtoull(s.substr(16 * i, 16).c_str(), nullptr, 16);
    const Fr r2{{Fr::R2[0], Fr::R2[1], Fr::R2[2], Fr::R2[3]}};
    return fr_mul(v, r2);
}

static std::string show(const Fr& m) {  // Montgomery -> canonical, 64 hex digits
    const Fr v = fr_mul(m, Fr{{1, 0, 0, 0}});
    char buf[65];
    snprintf(buf, sizeof(buf), "%016llx%016llx%016llx%016llx", (unsigned long long)v.l[3], (unsigned long long)v.l[2],
             (unsigned long long)v.l[1], (unsigned long long)v.l[0]);
    return buf;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1]);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string op;
        in >> op;
        if (op == "inv") {
            std::string a;
            in >> a;
            const Fr x = parse(a);
            if (!fr_is_canonical(x)) return 3;
            printf("inv %s\n", show(fr_inverse(x)).c_str());
        } else if (op == "add" || op == "sub") {
            std::string a, b;
            in >> a >> b;
            const Fr r = op == "add" ? fr_sum(parse(a), parse(b)) : fr_sub(parse(a), parse(b));
            if (!fr_is_canonical(r)) return 3;
            printf("%s %s\n", op.c_str(), show(r).c_str());
        } else if (op == "sel") {
            uint32_t log_n;
            std::string z;
            in >> log_n >> z;
            SelectorsAtPoint s;
            if (!selectors_at_point(log_n, parse(z), &s)) {
                printf("sel 0\n");
                continue;
            }
            printf("sel 1 %s %s %s %s\n", show(s.is_first_row).c_str(), show(s.is_last_row).c_str(),
                   show(s.is_transition).c_str(), show(s.inv_vanishing).c_str());
        } else if (op == "rec") {
            uint32_t log_n, log_qd;
            std::string z, c;
            in >> log_n >> log_qd >> z;
            std::vector<Fr> chunks;
            while (in >> c) chunks.push_back(parse(c));
            if (chunks.size() != (1u << log_qd)) return 4;
            printf("rec %s\n", show(recompose_quotient(log_n, log_qd, chunks.data(), parse(z))).c_str());
        } else if (!op.empty()) {
            return 5;
        }
    }
    return 0;
}
