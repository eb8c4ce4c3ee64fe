"""Corpus of the preset-dictionary tests and of tools/dict_time.py: small JSON
log records with fixed keys, the shape of data a shared dictionary is for.
dictionary() is 64 records of seed 1 joined; messages() are 4096 records of
seed 2.  Deterministic (random.Random only)."""
import json
import random

WORDS = ["request", "failed", "timeout", "retry", "connection", "closed", "user", "session",
         "cache", "miss", "upstream", "latency", "exceeded", "threshold", "completed", "queued"]
LEVELS = ["DEBUG", "INFO", "WARN", "ERROR"]
SERVICES = ["auth", "billing", "search", "gateway", "storage", "notify"]
TAGS = ["prod", "canary", "eu-west", "us-east", "batch", "edge", "internal", "v2"]


def record(rng, k):
    r = {
        "id": rng.getrandbits(48),
        "timestamp": "2024-%02d-%02dT%02d:%02d:%02d.%03dZ" % (rng.randint(1, 12), rng.randint(1, 28), rng.randint(0, 23),
                                                             rng.randint(0, 59), rng.randint(0, 59), rng.randint(0, 999)),
        "level": rng.choice(LEVELS),
        "service": rng.choice(SERVICES),
        "host": "%s-%02d.dc%d.example.net" % (rng.choice(SERVICES), rng.randint(0, 63), rng.randint(1, 4)),
        "message": " ".join(rng.choice(WORDS) for _ in range(rng.randint(4, 40))),
        "tags": rng.sample(TAGS, rng.randint(1, 3)),
        "latency": round(rng.uniform(0.1, 2500.0), 3),
        "ok": rng.random() < 0.8,
    }
    return json.dumps(r, sort_keys=True).encode()


def records(seed, count):
    rng = random.Random(seed)
    return [record(rng, k) for k in range(count)]


def dictionary():
    return b"".join(records(1, 64))


def messages(count=4096):
    return records(2, count)
