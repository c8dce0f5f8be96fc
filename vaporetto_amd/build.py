"""Builds libvaporetto_hip.so (HIP kernels + C ABI) in-tree for gfx950 with hipcc.

`python -m vaporetto_amd.build` or `__graft_entry__.build()`.  The .so is git-ignored but travels with the
gpurun snapshot; hipcc cross-compiles without a GPU.
"""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_DIR = os.path.join(HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libvaporetto_hip.so")
SOURCES = ["model.cpp", "tables.cpp", "capi.cpp", "capi_device.cpp", "capi_host.cpp", "kernels.hip", "kernels_fast.hip", "kernels_tags.hip", "kernels_emit.hip", "kernels_tokens.hip", "kernels_token_filter.hip", "kernels_vocab.hip", "kernels_vocab_count.hip", "kernels_postings.hip", "kernels_postings_merge.hip", "kernels_postings_search.hip", "kernels_postings_phrase.hip", "kernels_postings_boolean.hip", "kernels_listing.hip", "kernels_graphemes.hip", "pattern_tagger.cpp", "kernels_pattern.hip", "capi_parse.cpp", "kernels_parse.hip", "capi_train.cpp", "kernels_train.hip", "kernels_train_tags.hip", "kernels_train_l1.hip", "kernels_train_tags_l1.hip", "kernels_train_l1lr.hip", "kernels_train_tags_l1lr.hip"]
HEADERS = ["model.hpp", "tables.hpp", "layout.h", "tron.h", "l1r.h", "l1r_lr.h", "l1r_team.h", "kernels.hpp", "tag_records.h", "tag_vocab.hpp", "tag_stop.hpp", "device_common.h", "emit_common.h", "capi_internal.hpp", "host_chunks.hpp", "scratch_carve.hpp", "patset.hpp", "pattern_tagger.hpp", "vocab_table.hpp", "vocab_count.hpp", "vocab_resolve.h", "postings_score.h", os.path.join("..", "..", "include", "vaporetto_hip.h")]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function"]


def _stale() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(os.path.join(CSRC, f)) > t for f in SOURCES + HEADERS)


def build_hip(force: bool = False, verbose: bool = False, extra_flags=()) -> str:
    if not force and not _stale():
        return LIB_PATH
    os.makedirs(LIB_DIR, exist_ok=True)
    cmd = [HIPCC] + FLAGS + list(extra_flags) + ["-o", LIB_PATH] + SOURCES
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd, cwd=CSRC)
    return LIB_PATH


if __name__ == "__main__":
    print(build_hip(force="--force" in sys.argv, verbose=True))
