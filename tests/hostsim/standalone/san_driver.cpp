// san_driver — ONE call of one entry point of the host simulation under the compiler's sanitizers (TEST INFRASTRUCTURE ONLY).
// A program of its own: no Python in the process, nothing preloaded.  tests/hostsim/simdevice.py (build_standalone) links it
// with the rewritten sources of the simulated units and sim_runtime.cpp, everything compiled with
// -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all.
//
//   san_driver CASE_DIR
//
// CASE_DIR/manifest.txt, one record per line:
//   entry NAME                     the entry point (C ABI of include/xclim_hip.h)
//   buf ID NBYTES                  a memory block: CASE_DIR/ID.in holds its NBYTES bytes (raw, little-endian arrays)
//   arg ctx | i VALUE | d VALUE | n | p ID OFFSET | v K (ID OFFSET | -)...
//                                  the arguments in ABI order: the context of xh_create, an integer, a double (any strtod form,
//                                  hexadecimal included), NULL, a pointer OFFSET bytes into block ID, an array of K such pointers
// Every block is copied into a malloc block of EXACTLY NBYTES bytes — no padding, no rounding: a field of T rows of C cells is
// T * C elements unless the caller's view has a row stride — so that a read or write one element past the last cell of the last
// row lands in a redzone.  After the call every block is written back to CASE_DIR/ID.out and CASE_DIR/result.txt receives the
// return code and xh_last_error().  Exit status 0 = the call returned (whatever its code); a sanitizer report aborts.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "xclim_hip.h"

namespace {

struct Buf {
  std::string id;
  size_t n = 0;
  unsigned char* p = nullptr;
};
struct Arg {
  char kind = 'n';  // c ctx, i integer, d double, n NULL, p pointer, v pointer array
  long long i = 0;
  double d = 0;
  void* p = nullptr;
};

xh_ctx* g_ctx = nullptr;
std::vector<Arg> g_args;

[[noreturn]] void die(const char* what, const std::string& s) {
  fprintf(stderr, "san_driver: %s %s\n", what, s.c_str());
  exit(2);
}

// the K-th argument as the type the prototype declares at that position
template <typename T>
T get(size_t k) {
  if (k >= g_args.size()) die("too few arguments in the manifest for", "the entry point");
  const Arg& a = g_args[k];
  if constexpr (std::is_pointer_v<T>) {
    if (a.kind == 'c') return (T)g_ctx;
    if (a.kind != 'p' && a.kind != 'n' && a.kind != 'v') die("argument is not a pointer:", std::to_string(k));
    return (T)a.p;
  } else if constexpr (std::is_floating_point_v<T>) {
    if (a.kind != 'd' && a.kind != 'i') die("argument is not a number:", std::to_string(k));
    return a.kind == 'd' ? (T)a.d : (T)a.i;
  } else {
    if (a.kind != 'i') die("argument is not an integer:", std::to_string(k));
    return (T)a.i;
  }
}

template <typename... A, size_t... K>
int call_with(int (*f)(A...), std::index_sequence<K...>) {
  if (g_args.size() != sizeof...(A)) die("wrong number of arguments in the manifest for", "the entry point");
  return f(get<A>(K)...);
}
template <typename... A>
int call(int (*f)(A...)) {
  return call_with(f, std::index_sequence_for<A...>{});
}

#define XH_ENTRY(name) {#name, [] { return call(name); }}
const std::map<std::string, int (*)()> ENTRIES = {
    XH_ENTRY(xh_fire_weather),        XH_ENTRY(xh_overwintering_dc),    XH_ENTRY(xh_mcarthur),
    XH_ENTRY(xh_solar_table),         XH_ENTRY(xh_pet_month_table),     XH_ENTRY(xh_pet_daily),
    XH_ENTRY(xh_pet_monthly),         XH_ENTRY(xh_si_fit),              XH_ENTRY(xh_si_apply),
    XH_ENTRY(xh_si_fit_f64),          XH_ENTRY(xh_si_apply_f64),        XH_ENTRY(xh_thresholded_reduce_f64),
    XH_ENTRY(xh_range_reduce_f64),    XH_ENTRY(xh_domain_count_f64),    XH_ENTRY(xh_bivariate_count_f64),
    XH_ENTRY(xh_rolling_reduce_f64),  XH_ENTRY(xh_compare_map_f64),     XH_ENTRY(xh_run_stats_f64),
    XH_ENTRY(xh_spell_mask_f64),      XH_ENTRY(xh_spell_run_stats_f64), XH_ENTRY(xh_run_stats_doy_f64),
    XH_ENTRY(xh_percentile_doy_f64),
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) die("usage:", "san_driver CASE_DIR");
  const std::string dir = argv[1];
  FILE* mf = fopen((dir + "/manifest.txt").c_str(), "r");
  if (!mf) die("cannot open", dir + "/manifest.txt");
  std::string entry;
  std::vector<Buf> bufs;
  std::vector<std::vector<void*>*> tables;
  auto find = [&](const std::string& id) -> Buf& {
    for (Buf& b : bufs)
      if (b.id == id) return b;
    die("unknown block", id);
  };
  char line[1 << 16];
  while (fgets(line, sizeof line, mf)) {
    std::vector<std::string> w;
    for (char* t = strtok(line, " \t\r\n"); t; t = strtok(nullptr, " \t\r\n")) w.push_back(t);
    if (w.empty()) continue;
    if (w[0] == "entry" && w.size() == 2) {
      entry = w[1];
    } else if (w[0] == "buf" && w.size() == 3) {
      Buf b;
      b.id = w[1];
      b.n = (size_t)strtoull(w[2].c_str(), nullptr, 10);
      b.p = (unsigned char*)malloc(b.n);  // EXACTLY the block: the sanitizer's redzone starts at its last byte + 1
      FILE* f = fopen((dir + "/" + b.id + ".in").c_str(), "rb");
      if (!f || fread(b.p, 1, b.n, f) != b.n) die("cannot read block", b.id);
      fclose(f);
      bufs.push_back(b);
    } else if (w[0] == "arg" && w.size() >= 2) {
      Arg a;
      a.kind = w[1][0];
      if (w[1] == "ctx") a.kind = 'c';
      else if (w[1] == "i" && w.size() == 3) a.i = strtoll(w[2].c_str(), nullptr, 10);
      else if (w[1] == "d" && w.size() == 3) a.d = strtod(w[2].c_str(), nullptr);
      else if (w[1] == "n") a.p = nullptr;
      else if (w[1] == "p" && w.size() == 4) a.p = find(w[2]).p + strtoull(w[3].c_str(), nullptr, 10);
      else if (w[1] == "v" && w.size() >= 3) {
        auto* tab = new std::vector<void*>();
        size_t k = 3;
        for (long n = strtol(w[2].c_str(), nullptr, 10); n > 0; --n) {
          if (k >= w.size()) die("short pointer array in", entry);
          if (w[k] == "-") { tab->push_back(nullptr); k += 1; }
          else {
            if (k + 1 >= w.size()) die("short pointer array in", entry);
            tab->push_back(find(w[k]).p + strtoull(w[k + 1].c_str(), nullptr, 10));
            k += 2;
          }
        }
        tables.push_back(tab);
        a.p = tab->data();
      } else die("bad argument record", w[1]);
      g_args.push_back(a);
    } else die("bad manifest record", w[0]);
  }
  fclose(mf);
  const auto it = ENTRIES.find(entry);
  if (it == ENTRIES.end()) die("unknown entry point", entry);
  if (xh_create(0, &g_ctx) != XH_OK) die("xh_create failed", "");
  const int rc = it->second();
  for (const Buf& b : bufs) {
    FILE* f = fopen((dir + "/" + b.id + ".out").c_str(), "wb");
    if (!f || fwrite(b.p, 1, b.n, f) != b.n) die("cannot write block", b.id);
    fclose(f);
    free(b.p);
  }
  for (auto* t : tables) delete t;
  FILE* rf = fopen((dir + "/result.txt").c_str(), "w");
  if (!rf) die("cannot write", dir + "/result.txt");
  fprintf(rf, "%d\n%s\n", rc, rc != XH_OK ? xh_last_error() : "");
  fclose(rf);
  xh_destroy(g_ctx);
  return 0;
}
