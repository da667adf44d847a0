// aq_la_req.h -- the request order of the look-ahead sweep kernel's deep operand prefetch (aq_la_matrix.h), as two constexpr
// functions.  Plain C++, no HIP header: the kernel takes its vmcnt counts from them at compile time and a host program can
// include them to print what the kernel is built with (tests/test_host_logic.py).
#pragma once

// Operand prefetch with D buffers per stream (tile k in buffer k % D).  Request order of a phase: the tiles left dangling by the
// phase before -- [XU0 XA0 XU1 XA1 ...], XU up to tile D-2, XA up to D-3 -- then per step t: XU(t+D-1), XA(t+D-2) while they
// exist.  aq_req_index = position of a request in that order, aq_req_issued = requests out after the issues of step t; a wait
// for a tile is vmcnt(2 x (requests issued after it)): two loads per request, completed in order.
constexpr int aq_req_index(int D, int last, int stream /* 0 XU, 1 XA */, int k) {
  int n = 0;
  for (int j = 0; j <= D - 2; j++) {
    if (stream == 0 && k == j) return n;
    n++;
    if (j <= D - 3) {
      if (stream == 1 && k == j) return n;
      n++;
    }
  }
  for (int t = 0; t <= last; t++) {
    if (t + D - 1 <= last) {
      if (stream == 0 && k == t + D - 1) return n;
      n++;
    }
    if (t + D - 2 <= last) {
      if (stream == 1 && k == t + D - 2) return n;
      n++;
    }
  }
  return -1;
}
constexpr int aq_req_issued(int D, int last, int t) {
  int n = (D - 1) + (D - 2);
  for (int s = 0; s <= t; s++) n += (s + D - 1 <= last) + (s + D - 2 <= last);
  return n;
}
