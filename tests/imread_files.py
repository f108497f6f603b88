"""JPEG files the device image reader's tests build from a golden's bytes (tests/test_gpu_imread.py on the GPU,
tests/test_imread_cpu.py for the host-side split): no Pillow, plain marker surgery."""
import glob
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IMAGES = os.path.join(GOLDEN, "images")
EDGES = os.path.join(GOLDEN, "imread_dev")


def golden(name):
    with open(os.path.join(IMAGES, name), "rb") as f:
        return f.read()


def golden_jpegs():
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(IMAGES, "*.jpg")))


def edge_jpegs():
    """the fixture set of tests/golden/make_imread_dev_fixtures.py without the tools' two query frames"""
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(EDGES, "*.jpg"))
                  if not os.path.basename(p).startswith("query_"))


def segments(data):
    """[(marker, payload)] of the header segments up to and including SOS, and the entropy-coded rest"""
    assert data[:2] == b"\xff\xd8"
    out, p = [], 2
    while True:
        assert data[p] == 0xFF, p
        m = data[p + 1]
        n = (data[p + 2] << 8) | data[p + 3]
        out.append((m, data[p + 4:p + 2 + n]))
        p += 2 + n
        if m == 0xDA:
            return out, data[p:]


def assemble(segs, rest):
    out = bytearray(b"\xff\xd8")
    for m, payload in segs:
        n = len(payload) + 2
        out += bytes([0xFF, m, n >> 8, n & 255]) + payload
    return bytes(out + rest)


def with_16bit_quant_of_65535(data):
    """every DQT table replaced by a 16-bit table whose 64 entries are 65 535: dequantised coefficients leave 32 bits"""
    segs, rest = segments(data)
    out = []
    for m, payload in segs:
        if m == 0xDB:
            new, p = bytearray(), 0
            while p < len(payload):
                pq, tq = payload[p] >> 4, payload[p] & 15
                p += 1 + (128 if pq else 64)
                new += bytes([0x10 | tq]) + b"\xff" * 128
            payload = bytes(new)
        out.append((m, payload))
    return assemble(out, rest)


def as_rgb_file(data):
    """APP0 (JFIF) removed and the component ids set to R G B in SOF and SOS: libjpeg then skips the colour conversion"""
    segs, rest = segments(data)
    out = []
    for m, payload in segs:
        if m == 0xE0:
            continue
        payload = bytearray(payload)
        if m in (0xC0, 0xC1, 0xC2):
            assert payload[5] == 3
            old = [payload[6 + 3 * i] for i in range(3)]
            for i, c in enumerate(b"RGB"):
                payload[6 + 3 * i] = c
        if m == 0xDA:
            for i in range(payload[0]):
                payload[1 + 2 * i] = b"RGB"[old.index(payload[1 + 2 * i])]
        out.append((m, bytes(payload)))
    return assemble(out, rest)
