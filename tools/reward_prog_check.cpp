// Host sanitizer harness for the reward programs' validator and host interpreter
// (mujocoposelearning_amd/csrc/hs_reward_prog.h): the code every user-written reward passes through before
// it reaches the device.  Built with -fsanitize=address,undefined by
// `make -C mujocoposelearning_amd/csrc asan-reward-prog` and run by tests/test_reward_program.py over good
// programs and malformed encodings.
// For each file given: whitespace-separated numbers
//   nq nv nu nbody  n_instr n_consts n_params n_states
//   5 * n_instr code words, n_consts constants, n_params parameters,
//   then for every field in RpField order its n_states * row values
// (the counts are taken as they are: the vectors are sized by what the file holds, and the validator is
// what has to refuse a count the limits do not admit).  Prints one line per file:
// "OK <value> ..." (%.17g, one per state) or "ERR <message>".
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "hs_reward_prog.h"

int main(int argc, char** argv) {
  for (int a = 1; a < argc; a++) {
    std::ifstream in(argv[a]);
    hs::RpDims d{};
    long long n_instr = 0, n_consts = 0, n_params = 0, n_states = 0;
    if (!(in >> d.nq >> d.nv >> d.nu >> d.nbody >> n_instr >> n_consts >> n_params >> n_states) || d.nq < 0 ||
        d.nv < 0 || d.nu < 0 || d.nbody < 0 || n_states < 0 || n_states > 100000) {
      std::printf("ERR cannot read the header of %s\n", argv[a]);
      continue;
    }
    auto count = [](long long n) { return (size_t)(n < 0 ? 0 : n > 1000000 ? 1000000 : n); };
    std::vector<int32_t> code(5 * count(n_instr));
    std::vector<double> consts(count(n_consts)), params(count(n_params));
    bool ok = true;
    for (auto& c : code) ok = ok && (in >> c);
    for (auto& c : consts) ok = ok && (in >> c);
    for (auto& c : params) ok = ok && (in >> c);
    std::vector<std::vector<double>> fields(hs::RP_NFIELDS);
    for (int f = 0; f < hs::RP_NFIELDS && ok; f++) {
      fields[f].resize((size_t)n_states * hs::rp_field_len(d, f));
      for (auto& v : fields[f]) {
        std::string tok;   // "nan" / "inf" are not numbers to operator>>
        ok = ok && (in >> tok);
        if (ok) v = std::strtod(tok.c_str(), nullptr);
      }
    }
    if (!ok) {
      std::printf("ERR %s is truncated\n", argv[a]);
      continue;
    }
    hs::RpInfo info;
    const std::string why =
        hs::rp_validate(d, code.data(), (int)n_instr, consts.data(), (int)n_consts, (int)n_params, &info);
    if (!why.empty()) {
      std::printf("ERR %s\n", why.c_str());
      continue;
    }
    const double* fp[hs::RP_NFIELDS];
    for (int f = 0; f < hs::RP_NFIELDS; f++) fp[f] = fields[f].data();
    std::vector<double> out((size_t)n_states);
    hs::rp_eval_host(d, code.data(), (int)n_instr, consts.data(), params.data(), (int)n_states, fp, out.data());
    std::printf("OK");
    for (double v : out) std::printf(" %.17g", v);
    std::printf("\n");
  }
  return 0;
}
