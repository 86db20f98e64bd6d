"""csrc/th_owned.h on the CPU: DevBuf, OwnedEvent, OwnedStream and Pipe against stubs of the HIP runtime that count what is live and abort on a second free
(tests/host/owned_main.cpp), built with the address and undefined-behaviour sanitizers and run as it is."""

import subprocess

import host_programs


def test_owning_types_free_once_and_everything(tmp_path):
    exe = host_programs.build("owned_main.cpp", tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    done = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert done.returncode == 0, done.stdout + done.stderr
    assert done.stdout.strip() == "owned ok"
    assert "Sanitizer" not in done.stderr and "runtime error" not in done.stderr, done.stderr
