// maplists_check.cpp -- CPU check of circom_cvm_amd/csrc/maplists.hpp (the lazy row lists of the
// non-linear signal map across rounds) against the plain recursion it memoises
// (apply_substitution_to_map, constraint_simplification.rs:369-377).
//
// One MapLists lives through all rounds, as in the engine: after every batch is added, random
// signals are resolved and compared with the unmemoised recursion -- so a memo entry made in an
// earlier round must never answer for a different (signal, bound) pair later.
// usage: maplists_check <seed> <rounds> <signals>; prints "ok <checks>" or the first mismatch.
//
// File mode, maplists_check --file <path>: the lists of a recorded run of the reference algorithm
// (tests/round_cases.py maplists_input, from pyref's own map).  The file holds the initial lists
// (count, then `signal length rows...` each), the number of rounds and per round its queries
// (`count signals...`: the signals the round substitutes) and its batch (count, then
// `from length keys...` per substitution, in rank order).  Per round the queries are resolved over the
// batches of the rounds before it, every non-empty list is printed as `round signal length rows...`,
// and the batch is added; the test compares the lines with what pyref's map held beyond its initial part.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>

#include "maplists.hpp"

using rs::MapLists;

static std::vector<uint32_t> naive(const MapLists &M, const MapLists::Lists &init, uint32_t x, size_t u) {
  std::vector<uint32_t> out;
  for (size_t b = 0; b < u; ++b) {
    const MapLists::Batch &B = M.batches[b];
    for (size_t j = 0; j < B.from.size(); ++j) {
      bool has = false;
      for (uint64_t t = B.ptr[j]; t < B.ptr[j + 1]; ++t) has |= B.keys[t] == x;
      if (!has) continue;
      auto it = init.find(B.from[j]);
      if (it != init.end()) out.insert(out.end(), it->second.begin(), it->second.end());
      const std::vector<uint32_t> r = naive(M, init, B.from[j], b);
      out.insert(out.end(), r.begin(), r.end());
    }
  }
  return out;
}

static int file_mode(const char *path) {
  std::ifstream in(path);
  MapLists::Lists truth;
  uint64_t n = 0, len = 0;
  uint32_t s = 0;
  in >> n;
  for (uint64_t i = 0; i < n; ++i) {
    in >> s >> len;
    std::vector<uint32_t> l(len);
    for (auto &r : l) in >> r;
    truth[s] = l;
  }
  MapLists M;
  auto query = [&](const std::vector<uint32_t> &sigs) {
    for (uint32_t q : sigs) {
      if (M.minit.count(q)) continue;
      auto it = truth.find(q);
      M.minit[q] = it == truth.end() ? std::vector<uint32_t>() : it->second;
    }
  };
  uint64_t rounds = 0;
  in >> rounds;
  for (uint64_t r = 0; r < rounds; ++r) {
    in >> n;
    std::vector<uint32_t> X(n);
    for (auto &x : X) in >> x;
    const MapLists::Lists got = M.resolve(X, query);
    for (uint32_t x : X) {
      auto it = got.find(x);
      if (it == got.end()) continue;
      printf("%llu %u %zu", (unsigned long long)r, x, it->second.size());
      for (uint32_t row : it->second) printf(" %u", row);
      printf("\n");
    }
    MapLists::Batch B;
    B.ptr.push_back(0);
    in >> n;
    for (uint64_t j = 0; j < n; ++j) {
      in >> s >> len;
      B.from.push_back(s);
      for (uint64_t t = 0; t < len; ++t) {
        uint32_t key;
        in >> key;
        B.keys.push_back(key);
      }
      B.ptr.push_back(B.keys.size());
    }
    M.add_batch(std::move(B));
  }
  if (!in) {
    printf("bad input file\n");
    return 1;
  }
  printf("done\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 2 && !strcmp(argv[1], "--file")) return file_mode(argv[2]);
  const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  const int rounds = argc > 2 ? atoi(argv[2]) : 6;
  const uint32_t S = argc > 3 ? (uint32_t)atoi(argv[3]) : 40;
  std::mt19937_64 rng(seed);
  // the "device": every signal's initial list (ascending rows), queried on demand
  MapLists::Lists truth;
  for (uint32_t s = 1; s < S; ++s) {
    std::vector<uint32_t> l;
    for (uint32_t r = 0; r < 30; ++r)
      if (rng() % 7 == 0) l.push_back(r);
    if (!l.empty()) truth[s] = l;
  }
  MapLists M;
  std::vector<bool> queried(S, false);
  auto query = [&](const std::vector<uint32_t> &sigs) {
    for (uint32_t s : sigs) {
      if (queried[s]) continue;
      queried[s] = true;
      auto it = truth.find(s);
      M.minit[s] = it == truth.end() ? std::vector<uint32_t>() : it->second;
    }
  };
  std::vector<bool> deleted(S, false);
  uint64_t checks = 0;
  for (int r = 0; r < rounds; ++r) {
    // a round's substitutions: distinct `from`s (never deleted before), RHS over other live signals
    MapLists::Batch B;
    B.ptr.push_back(0);
    std::vector<uint32_t> froms;
    for (uint32_t s = 1; s < S; ++s)
      if (!deleted[s] && rng() % 4 == 0) froms.push_back(s);
    std::vector<bool> is_from(S, false);
    for (uint32_t f : froms) is_from[f] = true;
    for (uint32_t f : froms) {
      std::vector<uint32_t> keys;
      for (uint32_t s = 1; s < S; ++s)
        if (!is_from[s] && !deleted[s] && rng() % 3 == 0) keys.push_back(s);
      B.from.push_back(f);
      B.keys.insert(B.keys.end(), keys.begin(), keys.end());
      B.ptr.push_back(B.keys.size());
    }
    for (uint32_t f : froms) deleted[f] = true;
    M.add_batch(std::move(B));
    // resolve a random handful, as a round asks for its turning substitutions' signals
    for (int q = 0; q < 4; ++q) {
      std::vector<uint32_t> X;
      for (uint32_t s = 1; s < S; ++s)
        if (rng() % 5 == 0) X.push_back(s);
      const MapLists::Lists got = M.resolve(X, query);
      for (uint32_t x : X) {
        const std::vector<uint32_t> want = naive(M, truth, x, M.batches.size());
        auto it = got.find(x);
        const std::vector<uint32_t> &g = it == got.end() ? std::vector<uint32_t>() : it->second;
        ++checks;
        if (g != want) {
          printf("mismatch: seed %llu round %d signal %u: got %zu entries, want %zu\n", (unsigned long long)seed, r, x, g.size(),
                 want.size());
          return 1;
        }
      }
    }
  }
  printf("ok %llu\n", (unsigned long long)checks);
  return 0;
}
