'use strict'
// Version-history corpus (test tooling): rows for ygm_version_take_v1 / ygm_version_restore_v1 from the image's yjs
// 13.5.16 bundle (tools/yjs_bundle.js), a seeded generator.
//   node tools/version_corpus.js tests/golden/version_v135.json.gz [seed]
// Each row: { family, state, version, take, restored, restored_nogc } (hex), with
//   doc           = Y.applyUpdate(new Y.Doc({ gc: false }), state)
//   take          = Y.encodeSnapshot(Y.snapshot(doc))
//   restored      = Y.encodeStateAsUpdate(Y.createDocFromSnapshot(doc, Y.decodeSnapshot(version), new Y.Doc()))
//   restored_nogc = the same into new Y.Doc({ gc: false })
// and "throws" in place of the restored bytes where yjs throws.  Families: general (text, map, array, nested and
// deleted nested types, XML; one session in four with gc on, so GC structs arise), text (flat text, 1- to 4-byte
// characters), pending (lost updates), subdoc, crafted (random clocks, client subsets, a delete set from another
// moment, a clock above the state's), edge (built one by one, see edgeRows) and align (one edge document under root
// names of 1..32 bytes: every source phase of the kernel's copies).
// Prints per family how many restored rows differ from the plain snapshot of the state, and checks every row on the
// host twin (tools/snapdev/versiondev.cpp): no row yjs answers may be refused.
const fs = require('fs')
const os = require('os')
const path = require('path')
const zlib = require('zlib')
const cp = require('child_process')
const Y = require(path.join(__dirname, 'yjs_bundle.js')).load()

function rng (seed) {
  let x = (seed >>> 0) || 1
  return () => { x ^= x << 13; x >>>= 0; x ^= x >>> 17; x ^= x << 5; x >>>= 0; return x / 4294967296 }
}
const hex = b => Buffer.from(b).toString('hex')
const ALPH = ['a', 'b', 'c', 'd', 'e', ' ', 'é', 'ß', '€', '中', '😀', '🎉', 'x']

// ---- encoded Snapshot V1 by hand: writeDeleteSet (Map order), writeStateVector (Map order)
function vu (out, v) { while (v > 127) { out.push(128 | (v % 128)); v = Math.floor(v / 128) } out.push(v) }
function encVersion (ds, sv) {   // ds: Map client -> [{clock, len}], sv: Map client -> clock
  const o = []
  vu(o, ds.size)
  ds.forEach((rs, c) => { vu(o, c); vu(o, rs.length); rs.forEach(r => { vu(o, r.clock); vu(o, r.len) }) })
  vu(o, sv.size)
  sv.forEach((k, c) => { vu(o, c); vu(o, k) })
  return Uint8Array.from(o)
}
const liveVersion = d => Y.encodeSnapshot(Y.snapshot(d))

function expect (state, version) {
  const fromState = gc => { const d = new Y.Doc({ gc }); Y.applyUpdate(d, state); return d }
  const take = Y.encodeSnapshot(Y.snapshot(fromState(true)))
  const one = gc => {
    try { return hex(Y.encodeStateAsUpdate(Y.createDocFromSnapshot(fromState(false), Y.decodeSnapshot(version), new Y.Doc({ gc })))) } catch (e) { return 'throws' }
  }
  return { state: hex(state), version: hex(version), take: hex(take), restored: one(true), restored_nogc: one(false) }
}

// ---- sessions: peers edit and sync; versions are taken live between the operations
function session (seed, maxOps, kind) {
  const R = rng(seed * 2654435761 + 4242)
  const ri = n => Math.floor(R() * n)
  const gc = ri(4) === 0
  const nPeers = kind === 'text' ? 1 + ri(3) : 1 + ri(3)
  const peers = []; const log = []; const versions = []
  for (let p = 0; p < nPeers; p++) {
    const d = new Y.Doc({ gc })
    d.clientID = 1 + ri(R() < 0.5 ? 200 : 0x7ffffff0)
    d.on('update', (u, origin, doc, tr) => { if (tr.local) log.push(u) })
    peers.push(d)
  }
  const str = n => { let s = ''; for (let i = 0; i < n; i++) s += ALPH[ri(ALPH.length)]; return s }
  const nested = []
  const ops = 4 + ri(maxOps)
  for (let o = 0; o < ops; o++) {
    const p = ri(nPeers); const d = peers[p]
    if (R() < 0.15) {
      const q = ri(nPeers)
      if (q !== p) Y.applyUpdate(peers[q], Y.encodeStateAsUpdate(d, Y.encodeStateVector(peers[q])), 'remote')
      continue
    }
    if (o < ops * 0.8 && R() < 0.25) versions.push(liveVersion(d))   // (later operations follow: the restored document is an older one)
    const k = kind === 'text' ? 0 : ri(13)
    d.transact(() => {
      if (kind === 'subdoc' && R() < 0.2) {
        const opts = [{}, { autoLoad: true }, { meta: { v: ri(9) } }, { gc: false }][ri(4)]
        const sd = new Y.Doc(Object.assign({ guid: 'sub-' + ri(1e9) }, opts))
        if (R() < 0.6) d.getMap('docs').set('d' + ri(3), sd)
        else { const a = d.getArray('subs'); if (a.length && R() < 0.3) a.delete(ri(a.length), 1); else a.insert(ri(a.length + 1), [sd]) }
      } else if (k < 5) {
        const t = d.getText('text')
        if (t.length > 0 && R() < 0.35) { const at = ri(t.length); t.delete(at, 1 + ri(Math.min(6, t.length - at))) }
        else t.insert(ri(t.length + 1), str(1 + ri(R() < 0.7 ? 4 : 14)), kind !== 'text' && R() < 0.1 ? { bold: true } : undefined)
      } else if (k < 8) {
        const a = d.getArray('arr')
        if (a.length > 0 && R() < 0.3) { const at = ri(a.length); a.delete(at, 1 + ri(Math.min(3, a.length - at))) }
        else {
          const v = ri(6)
          if (v < 3) a.insert(ri(a.length + 1), [ri(1000), str(2), { k: ri(10) }, [true, null]].slice(0, 1 + ri(4)))
          else {
            const item = v === 3 ? new Y.Map() : v === 4 ? new Y.Array() : new Y.Text()
            a.insert(ri(a.length + 1), [item]); nested.push([p, item])
            if (v === 3) { item.set('n', ri(100)); item.set('m', str(2)) } else if (v === 4) item.push([str(1), ri(9), ri(9)]); else item.insert(0, str(4))
          }
        }
      } else if (k < 10) {
        const m = d.getMap('map'); const key = 'k' + ri(4)
        if (R() < 0.2) m.delete(key); else m.set(key, R() < 0.5 ? ri(100) : str(2))
      } else if (k < 11) {
        const f = d.getXmlFragment('xml')
        if (f.length > 0 && R() < 0.3) f.delete(ri(f.length), 1)
        else { const e = new Y.XmlElement('p'); f.insert(ri(f.length + 1), [e]); e.setAttribute('l', String(ri(3))); const tx = new Y.XmlText(); e.insert(0, [tx]); tx.insert(0, str(3)) }
      } else if (nested.length) {
        const [q, t] = nested[ri(nested.length)]
        if (q === p && t.doc === d && !(t._item && t._item.deleted)) {
          if (t instanceof Y.Text) t.insert(ri(t.length + 1), str(2))
          else if (t instanceof Y.Array) { if (t.length && R() < 0.4) t.delete(0, 1); else t.push([ri(50)]) } else t.set('m' + ri(3), str(1))
        }
      }
    })
  }
  for (let p = 1; p < nPeers; p++) Y.applyUpdate(peers[0], Y.encodeStateAsUpdate(peers[p], Y.encodeStateVector(peers[0])), 'remote')
  return { peers, log, versions, R, ri, gc }
}

function sessionRows (family, seed, count, maxOps) {
  const rows = []
  for (let i = 0; rows.length < count; i++) {
    const kind = family === 'crafted' ? 'general' : family
    const s = session(seed * 100003 + i, maxOps, kind)
    if (!s.log.length || !s.versions.length) continue
    let state
    let versions = s.versions
    if (family === 'pending') {
      const kept = s.log.slice(); const k = 1 + s.ri(Math.min(3, kept.length - 1))
      for (let j = 0; j < k && kept.length > 1; j++) kept.splice(s.ri(kept.length), 1)
      state = Y.mergeUpdates(kept)
      // the versions a gc: false server took while the lossy stream arrived
      const obs = new Y.Doc({ gc: false }); versions = []
      kept.forEach((u, j) => { Y.applyUpdate(obs, u); if (j + 1 < kept.length && s.ri(3) === 0) versions.push(liveVersion(obs)) })
      if (!versions.length) continue
      // ... and the peers' own live versions: ahead of what arrived (yjs throws) or, with a deletion of lost content,
      // a delete set past the kept clocks (pending after the cut)
      versions = versions.slice(-2).concat(s.versions.slice(-1))
      // ... and the server's last version with a peer's later delete set (ranges past the kept clocks: a pending
      // delete set after the cut) and, with several clients, one of them left out (not causally closed)
      const last = Y.decodeSnapshot(versions[0]); const sv = new Map(last.sv)
      if (sv.size > 1 && s.ri(2)) sv.delete(Array.from(sv.keys())[s.ri(sv.size)])
      versions.push(encVersion(Y.decodeSnapshot(liveVersion(s.peers[0])).ds.clients, sv))
    } else state = s.ri(2) || family === 'subdoc' ? Y.mergeUpdates(s.log) : Y.encodeStateAsUpdate(s.peers[0])   // (a deleted sub-document cannot be written again)
    if (family !== 'crafted') {
      const vs = versions.slice(-4)
      for (const v of vs) if (rows.length < count) rows.push(Object.assign({ family }, expect(state, v)))
      continue
    }
    // crafted: the state's clocks cut at random, some clients left out or at 0, a delete set from another moment
    const full = Y.decodeSnapshot(liveVersion(s.peers[0]))
    const other = Y.decodeSnapshot(s.versions[s.ri(s.versions.length)])
    for (let j = 0; j < 3 && rows.length < count; j++) {
      const sv = new Map()
      full.sv.forEach((clock, client) => {
        const r = s.R()
        if (r < 0.15) return
        sv.set(client, r < 0.25 ? 0 : r < 0.35 ? clock : 1 + s.ri(clock))
      })
      if (j === 2 && s.ri(3) === 0 && sv.size) { const c = Array.from(sv.keys())[0]; sv.set(c, full.sv.get(c) + 1) }   // yjs throws
      const ds = s.ri(2) ? other.ds.clients : full.ds.clients
      rows.push(Object.assign({ family }, expect(state, encVersion(ds, sv))))
    }
  }
  return rows
}

// ---- the edge family
function oneDoc (gc, id, f) { const d = new Y.Doc({ gc }); d.clientID = id; f(d); return d }
const svOf = pairs => encVersion(new Map(), new Map(pairs))
function edgeRows () {
  const rows = []
  const add = (note, state, version) => rows.push(Object.assign({ family: 'edge', note }, expect(state, version)))
  const two = oneDoc(false, 7, d => { d.getText('t').insert(0, 'abc'); d.getText('t').insert(0, 'de') })
  add('cut at a struct boundary', Y.encodeStateAsUpdate(two), svOf([[7, 3]]))
  add('cut at clock 1', Y.encodeStateAsUpdate(two), svOf([[7, 1]]))
  add('clock equal to the state', Y.encodeStateAsUpdate(two), liveVersion(two))
  add('every client absent', Y.encodeStateAsUpdate(two), svOf([]))
  add('clock 0 only', Y.encodeStateAsUpdate(two), svOf([[7, 0]]))
  const sur = oneDoc(false, 9, d => d.getText('t').insert(0, 'a😀b🎉c'))
  add('cut inside a surrogate pair', Y.encodeStateAsUpdate(sur), svOf([[9, 2]]))
  add('cut inside the second pair', Y.encodeStateAsUpdate(sur), svOf([[9, 5]]))
  add('cut after a pair', Y.encodeStateAsUpdate(sur), svOf([[9, 3]]))
  const any = oneDoc(false, 11, d => d.getArray('a').insert(0, [1, 'two', { k: [1, 2, { z: null }] }, [3, [4]], 2.5, true]))
  for (const k of [1, 2, 3, 4, 5]) add('cut in ContentAny at ' + k, Y.encodeStateAsUpdate(any), svOf([[11, k]]))
  const json = Uint8Array.from([1, 1, 13, 0, 0x02, 1, 1, 0x6a, 3, 1, 0x31, 3, 0x22, 0x78, 0x22, 4, 0x6e, 0x75, 0x6c, 0x6c, 0])
  for (const k of [1, 2]) add('cut in ContentJSON at ' + k, json, svOf([[13, k]]))
  const del = oneDoc(true, 15, d => { d.getText('t').insert(0, 'abcdefgh'); d.getText('t').delete(1, 5) })
  for (const k of [2, 3, 6, 7]) add('cut in ContentDeleted at ' + k, Y.encodeStateAsUpdate(del), svOf([[15, k]]))
  const gcd = oneDoc(true, 17, d => {
    const m = new Y.Map(); d.getArray('a').insert(0, [m]); m.set('a', 1); m.set('b', 2); m.set('c', 'x'); m.set('d', 4)
    d.getArray('a').delete(0, 1); d.getArray('a').insert(0, ['tail'])
  })
  for (const k of [1, 2, 3, 4, 5, 6]) add('straddled GC struct at ' + k, Y.encodeStateAsUpdate(gcd), svOf([[17, k]]))
  const pair = oneDoc(false, 21, d => d.getText('t').insert(0, 'one'))
  const pair2 = oneDoc(false, 22, d => d.getText('t').insert(0, 'two'))
  Y.applyUpdate(pair, Y.encodeStateAsUpdate(pair2))
  add('a client at clock 0', Y.encodeStateAsUpdate(pair), svOf([[21, 2], [22, 0]]))
  add('a client absent', Y.encodeStateAsUpdate(pair), svOf([[22, 3]]))
  const long = oneDoc(false, 23, d => d.getText('t').insert(0, 'a'.repeat(200)))
  add('string of 200 bytes cut to 100', Y.encodeStateAsUpdate(long), svOf([[23, 100]]))
  add('string of 200 bytes cut to 127', Y.encodeStateAsUpdate(long), svOf([[23, 127]]))
  const many = oneDoc(false, 25, d => { for (let i = 0; i < 130; i++) d.getText('t').insert(0, String.fromCharCode(97 + i % 26)) })
  add('130 structs cut to 5', Y.encodeStateAsUpdate(many), svOf([[25, 5]]))
  add('130 structs cut to 127', Y.encodeStateAsUpdate(many), svOf([[25, 127]]))
  add('130 structs cut to 128', Y.encodeStateAsUpdate(many), svOf([[25, 128]]))
  add('the empty document', Uint8Array.from([0, 0]), Uint8Array.from([0, 0]))
  const R = rng(77)
  for (const n of [1, 2, 63, 64, 65, 300]) {
    const all = new Y.Doc({ gc: false }); all.clientID = 5000
    const clocks = []
    for (let c = 0; c < n; c++) {
      const d = oneDoc(false, 100 + 3 * c, x => { x.getText('t').insert(0, 'p' + c); if (c % 3 === 0) x.getText('t').delete(0, 1) })
      Y.applyUpdate(all, Y.encodeStateAsUpdate(d))
      clocks.push([100 + 3 * c, Math.floor(R() * 4) % (2 + String(c).length)])
    }
    add(n + ' clients', Y.encodeStateAsUpdate(all), svOf(clocks))
    add(n + ' clients, live version', Y.encodeStateAsUpdate(all), liveVersion(all))
  }
  return rows
}
// one edge document (a cut surrogate pair inside a long string, a second client, a delete set) under root names of
// 1..32 bytes: the kept runs start at every source phase mod 16
function alignRows () {
  const rows = []
  for (let i = 1; i <= 32; i++) {
    const name = 'r' + 'x'.repeat(i - 1)
    const a = oneDoc(false, 31, d => { d.getText(name).insert(0, 'The quick brown fox 😀 jumps over the lazy dog, twice. '.repeat(3)); d.getText(name).delete(3, 4) })
    const b = oneDoc(false, 32, d => d.getText(name).insert(0, 'second client text'))
    Y.applyUpdate(a, Y.encodeStateAsUpdate(b))
    const ds = Y.decodeSnapshot(liveVersion(a)).ds.clients
    rows.push(Object.assign({ family: 'align' }, expect(Y.encodeStateAsUpdate(a), encVersion(ds, new Map([[31, 21 + 57], [32, 7]])))))
  }
  return rows
}

// ---- the host twin over every row
function twin (rows) {
  const dir = fs.mkdtempSync(path.join(os.tmpdir(), 'vcorpus-'))
  const exe = path.join(dir, 'versiondev'); const inp = path.join(dir, 'in.bin'); const out = path.join(dir, 'out.bin')
  cp.execFileSync('g++', ['-O1', '-std=c++17', '-o', exe, path.join(__dirname, 'snapdev', 'versiondev.cpp')])
  const parts = [Buffer.from(new Uint32Array([rows.length]).buffer)]
  for (const r of rows) for (const k of ['state', 'version']) { const b = Buffer.from(r[k], 'hex'); parts.push(Buffer.from(new Uint32Array([b.length]).buffer), b) }
  fs.writeFileSync(inp, Buffer.concat(parts))
  cp.execFileSync(exe, [inp, out, '1'])
  const b = fs.readFileSync(out); const st = []
  for (let i = 0, k = 0; i < b.length; k++) { const s = b.readInt32LE(i); const l = b.readUInt32LE(i + 4); i += 8 + l; if (k % 4 === 2) st.push(s) }
  return st
}

if (require.main === module) {
  const out = process.argv[2]
  const seed = parseInt(process.argv[3] || '1', 10)
  let rows = []
  rows = rows.concat(sessionRows('general', seed, 60, 40), sessionRows('text', seed + 1, 45, 40), sessionRows('pending', seed + 2, 60, 40),
    sessionRows('subdoc', seed + 3, 36, 40), sessionRows('crafted', seed + 4, 60, 40), edgeRows(), alignRows())
  const plain = u => { const d = new Y.Doc(); Y.applyUpdate(d, Buffer.from(u, 'hex')); return hex(Y.encodeStateAsUpdate(d)) }
  const fam = {}
  for (const r of rows) {
    const f = fam[r.family] = fam[r.family] || { rows: 0, throws: 0, differ_from_snapshot: 0 }
    f.rows++
    if (r.restored === 'throws') f.throws++
    else if (r.restored !== plain(r.state)) f.differ_from_snapshot++
  }
  console.log(JSON.stringify(fam))
  for (const k of Object.keys(fam)) {
    if (k !== 'edge' && k !== 'align' && fam[k].differ_from_snapshot * 10 < (fam[k].rows - fam[k].throws) * 9) throw new Error('family ' + k + ': too few rows differ from the plain snapshot')
  }
  const st = twin(rows)
  const pend = {}
  rows.forEach((r, i) => {
    if (r.restored !== 'throws' && st[i] !== 0 && st[i] !== 64) throw new Error('row ' + i + ' (' + r.family + ' ' + (r.note || '') + ') refused by the host twin: ' + st[i])
    if (st[i] === 64) pend[r.family] = (pend[r.family] || 0) + 1
  })
  console.log(JSON.stringify({ pending_after_the_cut: pend }))
  if (!pend.pending || !pend.crafted) throw new Error('the pending and crafted families must leave pending parts after the cut')
  fs.writeFileSync(out, zlib.gzipSync(Buffer.from(JSON.stringify({ yjs: '13.5.16', seed, rows })), { level: 9 }))
  console.log(JSON.stringify({ rows: rows.length, bytes: fs.statSync(out).size }))
}

module.exports = { session, encVersion }
