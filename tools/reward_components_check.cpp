// Host sanitizer harness for reward programs with named components (mujocoposelearning_amd/csrc/hs_reward_prog.h:
// RP_OUT, the validator's n_outputs and the host interpreter's component sink), the counterpart of
// reward_prog_check.cpp.  Built with -fsanitize=address,undefined by
// `make -C mujocoposelearning_amd/csrc asan-reward-components` and run by tests/test_reward_components.py over
// good programs and malformed encodings.
// For each file given: whitespace-separated numbers
//   nq nv nu nbody  n_instr n_consts n_params n_outputs n_states
//   5 * n_instr code words, n_consts constants, n_params parameters,
//   then for every field in RpField order its n_states * row values
// (the counts are taken as they are: the validator is what has to refuse a count the limits do not admit; the sink
// is sized by what the validator accepted).  Prints one line per file:
// "OK <reward> ... C <component> ..." (%.17g; one reward per state, then the components component-major,
// n_outputs * n_states values) or "ERR <message>".
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <limits>
#include <string>
#include <vector>

#include "hs_reward_prog.h"

int main(int argc, char** argv) {
  for (int a = 1; a < argc; a++) {
    std::ifstream in(argv[a]);
    hs::RpDims d{};
    long long n_instr = 0, n_consts = 0, n_params = 0, n_outputs = 0, n_states = 0;
    if (!(in >> d.nq >> d.nv >> d.nu >> d.nbody >> n_instr >> n_consts >> n_params >> n_outputs >> n_states) ||
        d.nq < 0 || d.nv < 0 || d.nu < 0 || d.nbody < 0 || n_states < 0 || n_states > 100000 ||
        n_outputs < -1000000 || n_outputs > 1000000) {
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
    const std::string why = hs::rp_validate(d, code.data(), (int)n_instr, consts.data(), (int)n_consts, (int)n_params,
                                            (int)n_outputs, &info);
    if (!why.empty()) {
      std::printf("ERR %s\n", why.c_str());
      continue;
    }
    const double* fp[hs::RP_NFIELDS];
    for (int f = 0; f < hs::RP_NFIELDS; f++) fp[f] = fields[f].data();
    std::vector<double> out((size_t)n_states);
    // exactly n_outputs rows, poisoned: a component the interpreter skipped or misplaced shows as NaN, a write
    // past the last row is the sanitizer's to find
    std::vector<double> comp((size_t)info.n_outputs * (size_t)n_states, std::numeric_limits<double>::quiet_NaN());
    hs::rp_eval_host(d, code.data(), (int)n_instr, consts.data(), params.data(), (int)n_states, fp, out.data(),
                     info.n_outputs > 0 ? comp.data() : nullptr);
    std::printf("OK");
    for (double v : out) std::printf(" %.17g", v);
    std::printf(" C");
    for (double v : comp) std::printf(" %.17g", v);
    std::printf("\n");
  }
  return 0;
}
