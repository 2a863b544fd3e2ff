"""Generate tests/golden/kfpkg_manifest.json from the reference's kfpkg/kpu_yolov3.kfpkg:

    python tests/golden/make_kfpkg_manifest.py <path to kpu_yolov3.kfpkg>

The manifest holds only data about the package: its file name, size and SHA-256, every zip member's name, size and CRC-32,
the SHA-256 of the `.kmodel` member that kmodel.read_kfpkg extracts, and the text of flash-list.json.  With it,
tests/test_kmodel.py checks that tests/golden/yolo.kmodel is that member, byte for byte, without the package itself.
"""
import hashlib
import json
import sys
import zipfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))


def main(path):
    from k210_yolo_framework_amd import kmodel
    path = Path(path)
    data = path.read_bytes()
    with zipfile.ZipFile(path) as z:
        members = [{'name': i.filename, 'size': i.file_size, 'crc32': i.CRC} for i in z.infolist()]
        flash_list = z.read('flash-list.json').decode()
    km = kmodel.read_kfpkg(path)
    manifest = {'package': path.name, 'package_size': len(data), 'package_sha256': hashlib.sha256(data).hexdigest(),
                'members': members, 'kmodel_sha256': hashlib.sha256(km).hexdigest(), 'kmodel_size': len(km),
                'flash_list_json': flash_list}
    Path(__file__).with_name('kfpkg_manifest.json').write_text(json.dumps(manifest, indent=1) + '\n')


if __name__ == '__main__':
    main(sys.argv[1])
