"""What the CPU tests of the scoring server (serve.py) share: a request assembled by hand from the documented layout, the small LP
snapshot and forced rows they send, a worker's end of a connection (`Peer`), a server over stubs that is driven without its loop
(`stub_server`, `server_fixture`) and one turn of that loop (`pump`).  The stub groups and sessions stay with the tests that
define what they log."""
import selectors
import socket
import struct

import numpy as np
import pytest

from gcnn_cut_selector_amd import lpstate, serve


def by_hand(kind, key, arrays, p_max=0.0, p_max_ub=0.0, max_selected=-1, n_forced=-1, a=0, b=0, c=0):
    """A request assembled from the documented layout alone: the header `<4sBBHddiiiii` (magic, kind, n_arrays, key length, p_max,
    p_max_ub, max_selected, n_forced and three words), the key, then per array a 24-byte descriptor `<BBHIIQ4x` (dtype code, rank,
    pad, two dimensions, byte count) and its raw buffer."""
    codes = {"float32": 0, "float64": 1, "int32": 2, "int64": 3, "uint8": 4, "int8": 5}
    out = [struct.pack("<4sBBHddiiiii", b"GCS1", kind, len(arrays), len(key), p_max, p_max_ub, max_selected, n_forced, a, b, c), key]
    for x in arrays:
        x = np.ascontiguousarray(x)
        shape = tuple(x.shape) + (0,) * (2 - x.ndim)
        out += [struct.pack("<BBHIIQ4x", codes[x.dtype.name], x.ndim, 0, shape[0], shape[1], x.nbytes), x.tobytes()]
    return b"".join(out)


def snap():
    return lpstate.LPSnapshot(
        row_ptr=np.array([0, 2, 3], np.int32), row_col=np.array([0, 2, 1], np.int32), row_val=np.array([1.0, -2.0, 0.5]),
        row_lhs=np.array([-1e20, 0.5]), row_rhs=np.array([3.0, 1e20]), row_dual=np.array([0.25, 0.0]), row_basis=np.array([0, 2], np.int8),
        col_type=np.array([0, 1, 3], np.int8), col_obj=np.array([1.0, 0.0, 2.0]), col_lb=np.zeros(3), col_ub=np.array([1.0, 1.0, 1e20]),
        col_basis=np.array([1, 0, 2], np.int8), col_lp=np.array([0.5, 1.0, 0.0]), col_redcost=np.array([0.0, 0.5, 0.0]),
        cut_ptr=np.array([0, 2, 3], np.int32), cut_col=np.array([0, 1, 2], np.int32), cut_val=np.array([1.0, 1.0, -1.0]),
        cut_lhs=np.array([-1e20, 0.25]), cut_rhs=np.array([1.5, 1e20]), col_primal=np.array([1.0, 0.0, 0.5]),
        col_primal_avg=np.array([0.5, 0.5, 0.5]))


FORCED = (np.array([[0, 0], [0, 2]], np.int32), np.array([1.0, -1.0], np.float32), 1)
BLOCK = lpstate.LPRowBlock(np.array([0, 1, 3], np.int32), np.array([2, 0, 1], np.int32), np.array([1.5, -1.0, 2.0]),
                           np.array([-1e20, 0.0]), np.array([2.0, 1e20]))


def same_fields(a, b, names):
    for n in names:
        x, y = getattr(a, n), getattr(b, n)
        assert (x is None and y is None) or np.array_equal(np.asarray(x), np.asarray(y)), n


class StubModel:
    """A model that only opens sessions: `session(model, rows, deep)` makes them, `opened` keeps them."""
    device = "stub"

    def __init__(self, name, session):
        self.name, self.session, self.opened = name, session, []

    def open_lp(self, rows, *, deep=True):
        self.opened.append(self.session(self, rows, deep))
        return self.opened[-1]


class Peer:
    """A worker's end of a connection to the server under test: sends framed messages, reads framed replies.  Usable as the
    `client` of a `RemoteLPSession`: `_call` sends a message, lets the server take one turn and reads the reply."""
    model_key = "a"

    def __init__(self, server):
        self.server = server
        self.sock, self.conn = socket.socketpair()
        self.sock.settimeout(5)              # a reply that does not come fails the test instead of blocking it
        server._buffers[self.conn] = bytearray()
        server._sel.register(self.conn, selectors.EVENT_READ)

    def send(self, message):
        self.sock.sendall(struct.pack("<I", len(message)) + message)

    def reply(self):
        (n,) = struct.unpack("<I", serve._recv_exact(self.sock, 4))
        return serve.decode_reply(serve._recv_exact(self.sock, n))

    def _call(self, message):
        self.send(message)
        pump(self.server, [self])
        return self.reply()


def stub_server(tmp_path, models, collector=None, **kw):
    """A `ScoringServer` over stub `models` (and a stub `collector`) with a selector but no loop: the test takes its turns with
    `pump`.  `kw` goes to the server (`max_sessions`, `session_group`)."""
    s = serve.ScoringServer(models, str(tmp_path / "sock"), **kw)
    s._collector = collector
    s._sel = selectors.DefaultSelector()
    return s


def shut(server):
    server._sel.close()
    server._shutdown()


def server_fixture(make):
    """A pytest fixture `server` from `make(tmp_path)`, which calls `stub_server` with the test module's own stubs."""
    @pytest.fixture
    def server(tmp_path):
        s = make(tmp_path)
        yield s
        shut(s)
    return server


def pump(server, peers):
    """What one turn of `serve_forever` does with what the peers have sent: read every connection, then serve."""
    pending, ready = [], {key.fileobj for key, _ in server._sel.select(0)}
    for p in peers:
        if p.conn in ready and p.conn in server._buffers:
            server._read(p.conn, pending)
    server._serve(pending)


def open_session(server, peer, key="a"):
    peer.send(serve.encode_open_request(key, lpstate.LPRows.from_snapshot(snap())))
    pump(server, [peer])
    return peer.reply()[1]
