#!/usr/bin/env python3
"""Data fixtures of the reference's test trees for tests/test_formats.py, cut so that they travel with the repository.

    python tests/golden/make_ref_fixtures.py <reference checkout>

Each 60 s float WAV (torchaudio layout: 18-byte fmt, fact, data; mono, 16 kHz, 960000 frames) becomes a one-second excerpt
around its loudest sample, cut at the byte level: the original 58-byte header with only its three size fields rewritten
(RIFF size, fact sample count, data size) and the original sample bytes, untouched.  json_data.json is copied verbatim.
MANIFEST.json records where every excerpt comes from.
"""
import hashlib
import json
import os
import shutil
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ref_fixtures")
WAVS = ["separation/tests/noise/s1.wav", "separation/tests/noise/s2.wav", "separation/tests/noise/mix.wav",
        "enhancement/tests/noise/s1.wav", "enhancement/tests/noise/mix.wav"]
JSON = "enhancement/tests/noise/json_data.json"
FRAMES = 16000


def local_name(rel):
    tree, _, _, name = rel.split("/")
    return f"{tree}_noise_{name}"


def main(ref):
    os.makedirs(OUT, exist_ok=True)
    manifest = {}
    for rel in WAVS:
        raw = open(os.path.join(ref, rel), "rb").read()
        hdr, data = raw[:58], np.frombuffer(raw[58:], dtype="<f4")
        assert hdr[36:42] == b"\0\0fact" and hdr[50:54] == b"data" and struct.unpack_from("<I", hdr, 54)[0] == 4 * data.size
        start = int(np.clip(int(np.argmax(np.abs(data))) - FRAMES // 2, 0, data.size - FRAMES))
        h = bytearray(hdr)
        struct.pack_into("<I", h, 4, 50 + 4 * FRAMES)
        struct.pack_into("<I", h, 46, FRAMES)
        struct.pack_into("<I", h, 54, 4 * FRAMES)
        excerpt = bytes(h) + raw[58 + 4 * start:58 + 4 * (start + FRAMES)]
        with open(os.path.join(OUT, local_name(rel)), "wb") as f:
            f.write(excerpt)
        manifest[rel] = {"file": local_name(rel), "frames": FRAMES, "first_frame": start, "source_frames": int(data.size),
                         "source_sha256": hashlib.sha256(raw).hexdigest()}
    shutil.copyfile(os.path.join(ref, JSON), os.path.join(OUT, local_name(JSON)))
    manifest[JSON] = {"file": local_name(JSON), "verbatim": True}
    with open(os.path.join(OUT, "MANIFEST.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
