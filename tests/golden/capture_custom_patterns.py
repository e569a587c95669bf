#!/usr/bin/env python3
"""Capture golden vectors for EDITED LogsAgent.error_patterns from the reference itself.

Run ONCE where the reference is checked out (the path capture_reference.py uses), in the manner of
capture_reference.py: `python tests/golden/capture_custom_patterns.py`.  Nothing on the GPU box
runs it and no reference source is copied: the output is data (inputs + expected outputs).

Writes logs_custom_patterns.json: for the pattern sets A, B and C of tests/custom_pattern_sets.py
  * the (name, regex) list,
  * 34 small container texts each (capture_reference's line generator plus lines for the set's own
    categories, case-mangled, with the Unicode hazards and every str.splitlines separator),
  * per line the category mask of re.search(regex, line, re.IGNORECASE),
  * per container the reference's own _analyze_container_logs output with error_patterns replaced
    (counts and the first three example lines sit in its findings' issue / evidence),
and the reference LogsAgent's analyze() result on its mock cluster (argument-order shim of
SURVEY.md §8c) with error_patterns replaced by set A.
"""
import os
import random
import re
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "kubernetes-rca-system_amd"))
import capture_reference as CR  # noqa: E402
from custom_pattern_sets import SETS  # noqa: E402

EXTRA = {
    "A": ["rpc error: context deadline exceeded", "context canceled by caller {w}", "request to {w} timed out after {n}ms",
          "Context Deadline Exceeded", "contextcanceled", "timeout waiting for {w}", "Timeout: {n}ms"],
    "B": ["quota exceeded for project {w}", "rate limit hit for {w}", "HTTP 429 Too Many Requests", "Quota  exceeded",
          "x509: certificate signed by unknown authority", "tls: handshake failure", "net/http: TLS handshake timeout",
          "write /data/{w}: No space left on device", "node {w} has disk pressure", "read /dev/sd{n}: I/O error",
          "X509: CERTIFICATE has expired", "I/O  error", "rate-limit", "428 Too Many Requests"],
    "C": ["java.lang.OutOfMemoryError: Java heap space", "javaxlangxOutOfMemoryError wildcard dots", "GC overhead limit exceeded",
          "GET /{w} HTTP/1.1\" 503 {n}", "HTTP/1.1\" 5٣٤ arabic-indic", "status=502 from {w}", "status=5x2", "STATUS=5{m}",
          "zookeeper session expired for /brokers/{w}", "KeeperErrorCode = ConnectionLoss", "KeeperErrorCode kelvin",
          "Keeper ErrorCode", "HTTP/1.1\" 404", "zookeeper ſeſſion expired long s"],
}


def masks_of(patterns, text):
    out = []
    for line in text.splitlines():
        m = 0
        for b, (_, p) in enumerate(patterns):
            if re.search(p, line, re.IGNORECASE):
                m |= 1 << b
        out.append(m)
    return out


def dump_compact(name, out):
    """One line per container (capture_reference.dump's indent=1 puts every mask on a line of its own)."""
    import json
    enc = lambda o: json.dumps(o, ensure_ascii=True, separators=(",", ":"))  # noqa: E731
    L = ['{"sets":{']
    for i, (k, v) in enumerate(out["sets"].items()):
        L.append(enc(k) + ':{"patterns":' + enc(v["patterns"]) + ',"containers":[')
        L += [enc(c) + ("," if j + 1 < len(v["containers"]) else "") for j, c in enumerate(v["containers"])]
        L.append("]}" + ("," if i + 1 < len(out["sets"]) else ""))
    L.append('},"mock_cluster_A":' + enc(out["mock_cluster_A"]) + "}")
    path = os.path.join(HERE, name)
    with open(path, "w") as f:
        f.write("\n".join(L) + "\n")
    print("wrote", path, os.path.getsize(path), "bytes")


def main():
    sys.dont_write_bytecode = True
    CR.install_stubs()
    sys.path.insert(0, CR.REF)
    os.chdir(tempfile.mkdtemp(prefix="krca_ref_"))  # the reference writes logs/ into the CWD
    from agents.logs_agent import LogsAgent  # noqa: E402
    from utils.mock_k8s_client import MockK8sClient  # noqa: E402

    class Shim(MockK8sClient):
        def get_recently_terminated_pods(self, namespace):
            return []

        def get_pod_logs(self, pod_name, namespace, container_name=None, tail_lines=100, previous=False):
            return MockK8sClient.get_pod_logs(self, namespace, pod_name, container_name, tail_lines, previous)

    base_templates = list(CR.ERR_TEMPLATES)
    out = {"sets": {}}
    for si, name in enumerate(("A", "B", "C")):
        patterns = [list(p) for p in SETS[name]]
        rng = random.Random(20260101 + si)
        CR.ERR_TEMPLATES = base_templates + EXTRA[name] * 3
        la = LogsAgent(CR.DictClient())
        la.error_patterns = dict(SETS[name])
        containers = []
        for ci in range(34):
            text = CR.gen_container_text(rng, rng.choice([1, 2, 3, 5, 8, 13, 21]))
            la.reset()
            la._analyze_container_logs("pod-%d" % ci, "c%d" % (ci % 3), text)
            containers.append({"pod": "pod-%d" % ci, "container": "c%d" % (ci % 3), "text": text,
                               "masks": masks_of(patterns, text), "result": CR.strip_ts(la.get_results())})
        out["sets"][name] = {"patterns": patterns, "containers": containers}
    CR.ERR_TEMPLATES = base_templates
    la = LogsAgent(Shim())
    la.error_patterns = dict(SETS["A"])
    out["mock_cluster_A"] = {"namespace": "test-microservices", "result": CR.strip_ts(la.analyze("test-microservices"))}
    dump_compact("logs_custom_patterns.json", out)


if __name__ == "__main__":
    main()
