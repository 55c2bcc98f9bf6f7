// gp_qacqf_columns.h -- the column packing of the value-layout joint passes (include/scaml_gp.h (5h), (7r)), stated once for the
// kernels, the host launcher, the host emulation and -- through scaml_qacqf_value_columns -- Python.
//
// B batches of q points are laid into strips of 16 columns so that no batch straddles a strip: the q x q diagonal blocks of a strip's
// Gram tile are then the batches' own covariances.  A strip holds bps = 16 / q whole batches (integer division); the 16 - bps q
// columns behind them are padding (none for q in {1, 2, 4, 8}; 1, 1, 4, 2 for q = 3, 5, 6, 7), and so are the columns of the last
// strip behind batch B - 1.  The points of a batch are consecutive columns.
#pragma once

namespace scaml {

constexpr int QAV_STRIP = 16;

constexpr int qav_batches_per_strip(int q) { return QAV_STRIP / q; }

// column of point j of batch b
constexpr int qav_column(int b, int j, int q) {
  return QAV_STRIP * (b / qav_batches_per_strip(q)) + (b % qav_batches_per_strip(q)) * q + j;
}

// Mp: columns of B batches, a multiple of 16
constexpr int qav_columns(int B, int q) {
  return QAV_STRIP * ((B + qav_batches_per_strip(q) - 1) / qav_batches_per_strip(q));
}

// the batch of local column c of strip `strip`, or -1 for a padding column
constexpr int qav_batch_of(int strip, int c, int q, int B) {
  return (c / q >= qav_batches_per_strip(q) || strip * qav_batches_per_strip(q) + c / q >= B) ? -1 : strip * qav_batches_per_strip(q) + c / q;
}

}  // namespace scaml
