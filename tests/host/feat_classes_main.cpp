// The stand-alone program of tests/test_feat_classes_host.py: open_vins_amd/csrc/feat_classes.h, which has no HIP in it, under the address and
// undefined-behaviour sanitizers.  Reads one batch per line from standard input — the track lengths in batch order, an empty line for an empty
// batch —, builds the offsets and the track order as begin_feature_batch does (a counting sort by descending length, equal lengths in batch
// order), and prints the partition: "n" and per class "kernel begin end m_max".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "feat_classes.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::vector<int32_t> offsets(1, 0);
    for (int m; in >> m;) offsets.push_back(offsets.back() + m);
    const int F = (int)offsets.size() - 1;
    int m_max = 0;
    for (int f = 0; f < F; f++) m_max = std::max(m_max, offsets[f + 1] - offsets[f]);
    std::vector<int32_t> start(m_max + 2, 0), order(F > 0 ? F : 1, 0);
    for (int f = 0; f < F; f++) start[m_max - (offsets[f + 1] - offsets[f]) + 1]++;
    for (int b = 0; b <= m_max; b++) start[b + 1] += start[b];
    for (int f = 0; f < F; f++) order[start[m_max - (offsets[f + 1] - offsets[f])]++] = f;
    const ovg::featcls::Partition pt = ovg::featcls::partition(offsets.data(), order.data(), F);
    std::printf("%d", pt.n);
    for (int k = 0; k < pt.n; k++) std::printf(" %d %d %d %d", pt.cls[k].kernel, pt.cls[k].begin, pt.cls[k].end, pt.cls[k].m_max);
    std::printf("\n");
  }
  return 0;
}
