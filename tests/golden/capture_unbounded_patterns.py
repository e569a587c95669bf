#!/usr/bin/env python3
"""Capture golden vectors for LogsAgent.error_patterns WITH UNBOUNDED QUANTIFIERS from the reference itself.

Run ONCE where the reference is checked out (the path capture_reference.py uses), in the manner of
capture_custom_patterns.py: `python tests/golden/capture_unbounded_patterns.py`.  Nothing on the GPU box
runs it and no reference source is copied: the output is data (inputs + expected outputs).

Writes logs_unbounded_patterns.json for set U1 of tests/unbounded_pattern_sets.py (the 13 shipped
patterns with exception -> Exception.*at):
  * the (name, regex) list,
  * 20 small container texts (capture_reference's line generator plus lines for the edited category:
    "Exception ... at" in order, out of order, case-mangled, across separators, with a long gap),
  * per line the category mask of re.search(regex, line, re.IGNORECASE),
  * per container the reference's own _analyze_container_logs output with error_patterns replaced,
and the reference LogsAgent's analyze() result on its mock cluster with error_patterns replaced by U1.
"""
import json
import os
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "kubernetes-rca-system_amd"))
import capture_reference as CR  # noqa: E402
from capture_custom_patterns import masks_of  # noqa: E402
from unbounded_pattern_sets import U1  # noqa: E402

EXTRA = ["java.lang.IllegalStateException: pool {w} closed at com.example.Pool.take(Pool.java:{n})",
         "Unhandled exception in worker {n} AT stage {m}", "at startup: Exception in {w}", "NullPointerException",
         "Exception at the next line", "EXCEPTION" + " {w}" * 60 + " at the far end", "exceptionat", "Exception a t",
         "ERROR: {w} failed", "Traceback (most recent call last):", "panic: runtime error at {w}"]


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

    patterns = [list(p) for p in U1]
    rng = random.Random(20260214)
    CR.ERR_TEMPLATES = list(CR.ERR_TEMPLATES) + EXTRA * 3
    la = LogsAgent(CR.DictClient())
    la.error_patterns = dict(U1)
    containers = []
    for ci in range(20):
        text = CR.gen_container_text(rng, rng.choice([1, 2, 3, 5, 8, 13]))
        la.reset()
        la._analyze_container_logs("pod-%d" % ci, "c%d" % (ci % 3), text)
        containers.append({"pod": "pod-%d" % ci, "container": "c%d" % (ci % 3), "text": text,
                           "masks": masks_of(patterns, text), "result": CR.strip_ts(la.get_results())})
    la = LogsAgent(Shim())
    la.error_patterns = dict(U1)
    out = {"patterns": patterns, "containers": containers,
           "mock_cluster": {"namespace": "test-microservices", "result": CR.strip_ts(la.analyze("test-microservices"))}}
    path = os.path.join(HERE, "logs_unbounded_patterns.json")
    with open(path, "w") as f:
        json.dump(out, f, ensure_ascii=True, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
