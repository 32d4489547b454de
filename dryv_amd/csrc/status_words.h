// status_words.h — how the host APIs (recon_api.hip, inter_api.hip) read the status words a kernel reports through: a few
// 32-bit words in device memory that the host clears in front of a submit and fetches where it waits.
#pragma once

namespace dryv {

enum StatusWord : unsigned {
  // the words
  kStatusFlags = 0,       // the bits below
  kStatusGaveUpTask = 1,  // with kStatusGaveUp: the band task that gave up waiting,
  kStatusGaveUpStep = 2,  //   its step << 16 | the macroblocks of the band above it needed,
  kStatusGaveUpSaw = 3,   //   and how many of them it saw
  kStatusFirstFlagged = 4,  // with kStatusBeyondInt32: ~(sequence number of the first queued batch that raised it)
  // the bits of word kStatusFlags
  kStatusUnsupported = 1u,  // a record outside the supported domain (its macroblock is zero-filled): DRYV_E_UNSUPPORTED
  kStatusBeyondInt32 = 2u,  // band kernel, fast build: a block beyond its 32-bit arithmetic; the host runs the batch again
                            //   with the wide build before anything is reported
  kStatusGaveUp = 4u,       // a band gave up waiting for the band above (every spin is bounded): DRYV_E_DEVICE
};

}  // namespace dryv
