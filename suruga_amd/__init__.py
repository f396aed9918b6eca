"""suruga_amd -- MI355X-native (gfx950) drop-in for suruga's record-layer
ChaCha20-Poly1305 AEAD (klutzy/suruga src/crypto + src/cipher).

Layout:
  include/suruga_gpu.h       C ABI (the drop-in boundary; at the repo root)
  suruga_amd/csrc/           gfx950 HIP kernels + C-ABI implementation
  suruga_amd/cipher.py       mirror of suruga's Aead/Encryptor/Decryptor traits
  suruga_amd/batch.py        device-resident batch seal/open (record-layer batching)
  suruga_amd/msg.py          one long message (any data / AD length) over the whole chip,
                             in the draft construction or (rfc8439=True) RFC 8439
  suruga_amd/tls13.py        TLS 1.3 protected stream (Tls13Writer / Tls13StreamReader) over
                             sg_write_records_tls13 / sg_read_records_tls13
  suruga_amd/quic.py         QUIC packet protection of a device-resident batch (RFC 9001):
                             AEAD and header protection, seal_quic / open_quic
  suruga_amd/wg.py           WireGuard transport data messages of a device-resident batch:
                             header, zero padding, AEAD and the inner length, seal_wg / open_wg
  suruga_amd/esp.py          IPsec ESP packets of a device-resident batch (RFC 7634): header, padding
                             and trailer, AEAD with the ESN additional data, seal_esp / open_esp
  suruga_amd/dtls13.py       DTLS 1.3 records of a device-resident batch (RFC 9147): unified header, inner
                             plaintext, AEAD and record number encryption, seal_dtls13 / open_dtls13
  suruga_amd/_native.py      ctypes binding of libsuruga_gpu.so

The HIP library is the only compute path; importing the cipher classes works
without a GPU, calling them needs one (and fails loudly otherwise).
"""
from . import _native
from .cipher import (Aead, ChaCha20Poly1305, ChaCha20Poly1305Decryptor, ChaCha20Poly1305Encryptor,
                     ChaCha20Poly1305Rfc8439, CipherSuite, Decryptor, Encryptor, TlsError, TlsErrorKind)
from .keysched import quic_packet_keys
from .quic import QuicBatch, decode_pn, open_quic, seal_quic
from .esp import EspBatch, open_esp, seal_esp
from .esp import packet_len as esp_packet_len, padded_len as esp_padded_len, seq_hi as esp_seq_hi
from .dtls13 import Dtls13Batch, open_dtls13, seal_dtls13
from .dtls13 import header_len as dtls13_header_len, inner_len as dtls13_inner_len
from .dtls13 import record_keys as dtls13_record_keys, record_len as dtls13_record_len
from .wg import SG_STATUS_BAD_HEADER, SG_STATUS_BAD_INNER, WgBatch, message_len, open_wg, padded_len, seal_wg

__all__ = [
    "Aead", "ChaCha20Poly1305", "ChaCha20Poly1305Decryptor", "ChaCha20Poly1305Encryptor", "ChaCha20Poly1305Rfc8439",
    "CipherSuite", "Decryptor", "Encryptor", "TlsError", "TlsErrorKind", "load_native",
    "QuicBatch", "seal_quic", "open_quic", "decode_pn", "quic_packet_keys",
    "WgBatch", "seal_wg", "open_wg", "padded_len", "message_len", "SG_STATUS_BAD_HEADER", "SG_STATUS_BAD_INNER",
    "EspBatch", "seal_esp", "open_esp", "esp_padded_len", "esp_packet_len", "esp_seq_hi",
    "Dtls13Batch", "seal_dtls13", "open_dtls13", "dtls13_header_len", "dtls13_inner_len", "dtls13_record_len",
    "dtls13_record_keys",
]


def load_native():
    """Load libsuruga_gpu.so (raises ImportError when it has not been built)."""
    return _native.load()
