'use strict'
// Version-history corpus, one state with many versions (test tooling): documents for ygm_version_restore_shared_v1 from
// the image's yjs 13.5.16 bundle (tools/yjs_bundle.js), a seeded generator modelled on tools/version_corpus.js.
//   node tools/version_history_corpus.js tests/golden/version_history_v135.json.gz [seed]
// Each document: { family, state, versions: [{ note?, version, restored, restored_nogc }] } (hex), the state taken from
// a gc: false Y.Doc at the end of its timeline, the versions taken with Y.snapshot between the edits, and
//   doc           = Y.applyUpdate(new Y.Doc({ gc: false }), state)
//   restored      = Y.encodeStateAsUpdate(Y.createDocFromSnapshot(doc, Y.decodeSnapshot(version), new Y.Doc()))
//   restored_nogc = the same into new Y.Doc({ gc: false })
// with "throws" in place of the restored bytes where yjs throws.  Families: text (one document typed into and deleted
// from, 48 versions), clients (three to five interleaved clients over map / array / xml content), many (300 clients),
// pending (a state that leaves pending structs), crafted (per document good versions, a version ahead of the state --
// yjs throws -- and a version taken from a different document), empty (the empty document with its single version) and
// large (one state of about 300 KB: what the chunked host API splits over several chunks).
// Prints the family counts, asserts that at least 90 % of the answered versions restore to bytes different from the
// plain snapshot of the state, and that the file is at most 400 KB.
const fs = require('fs')
const path = require('path')
const zlib = require('zlib')
const Y = require(path.join(__dirname, 'yjs_bundle.js')).load()

function rng (seed) {
  let x = (seed >>> 0) || 1
  return () => { x ^= x << 13; x >>>= 0; x ^= x >>> 17; x ^= x << 5; x >>>= 0; return x / 4294967296 }
}
const hex = b => Buffer.from(b).toString('hex')
const ALPH = ['a', 'b', 'c', 'd', 'e', ' ', 'é', 'ß', '€', '中', '😀', '🎉', 'x']
const liveVersion = d => Y.encodeSnapshot(Y.snapshot(d))

function restoreBoth (state, version) {
  const fromState = () => { const d = new Y.Doc({ gc: false }); Y.applyUpdate(d, state); return d }
  const one = gc => {
    try { return hex(Y.encodeStateAsUpdate(Y.createDocFromSnapshot(fromState(), Y.decodeSnapshot(version), new Y.Doc({ gc })))) } catch (e) { return 'throws' }
  }
  return { version: hex(version), restored: one(true), restored_nogc: one(false) }
}
function docRow (family, state, versions, notes) {
  return { family, state: hex(state), versions: versions.map((v, i) => Object.assign(notes && notes[i] ? { note: notes[i] } : {}, restoreBoth(state, v))) }
}
function newDoc (id) { const d = new Y.Doc({ gc: false }); d.clientID = id; return d }

// ---- text: one client typing and deleting, a version every few edits
function textDoc (seed, nVersions) {
  const R = rng(seed * 2654435761 + 17); const ri = n => Math.floor(R() * n)
  const d = newDoc(1 + ri(1 << 20)); const t = d.getText('text'); const versions = []
  const str = n => { let s = ''; for (let i = 0; i < n; i++) s += ALPH[ri(ALPH.length)]; return s }
  while (versions.length < nVersions) {
    for (let k = 0; k < 2 + ri(4); k++) {
      if (t.length > 4 && R() < 0.35) { const at = ri(t.length); t.delete(at, 1 + ri(Math.min(6, t.length - at))) } else t.insert(ri(t.length + 1), str(1 + ri(R() < 0.7 ? 4 : 14)))
    }
    versions.push(liveVersion(d))
  }
  for (let k = 0; k < 6; k++) t.insert(ri(t.length + 1), str(3))   // (later edits: every version is an older document)
  t.delete(0, 2)
  return docRow('text', Y.encodeStateAsUpdate(d), versions)
}

// ---- clients: interleaved clients over map / array / xml, synced now and then; versions taken on the first peer
function clientsDoc (seed, nPeers, nVersions) {
  const R = rng(seed * 2654435761 + 99); const ri = n => Math.floor(R() * n)
  const peers = []
  for (let p = 0; p < nPeers; p++) peers.push(newDoc(10 + 7 * p + ri(5) + (p & 1 ? 0x100000 : 0)))
  const str = n => { let s = ''; for (let i = 0; i < n; i++) s += ALPH[ri(ALPH.length)]; return s }
  const sync = (a, b) => Y.applyUpdate(b, Y.encodeStateAsUpdate(a, Y.encodeStateVector(b)), 'remote')
  const versions = []
  while (versions.length < nVersions) {
    for (let o = 0; o < 3 + ri(4); o++) {
      const d = peers[ri(nPeers)]; const k = ri(3)
      d.transact(() => {
        if (k === 0) { const m = d.getMap('map'); const key = 'k' + ri(4); if (R() < 0.2) m.delete(key); else m.set(key, R() < 0.5 ? ri(100) : str(2)) } else if (k === 1) {
          const a = d.getArray('arr')
          if (a.length > 0 && R() < 0.3) { const at = ri(a.length); a.delete(at, 1 + ri(Math.min(3, a.length - at))) } else a.insert(ri(a.length + 1), [ri(1000), str(2), { k: ri(10) }, [true, null]].slice(0, 1 + ri(4)))
        } else {
          const f = d.getXmlFragment('xml')
          if (f.length > 0 && R() < 0.3) f.delete(ri(f.length), 1)
          else { const e = new Y.XmlElement('p'); f.insert(ri(f.length + 1), [e]); e.setAttribute('l', String(ri(3))); const tx = new Y.XmlText(); e.insert(0, [tx]); tx.insert(0, str(3)) }
        }
      })
    }
    for (let p = 1; p < nPeers; p++) if (R() < 0.6) sync(peers[p], peers[0])
    if (R() < 0.3) sync(peers[0], peers[1 + ri(nPeers - 1)])
    versions.push(liveVersion(peers[0]))
  }
  for (let p = 1; p < nPeers; p++) sync(peers[p], peers[0])
  peers[0].getMap('map').set('last', 1)
  return docRow('clients', Y.encodeStateAsUpdate(peers[0]), versions)
}

// ---- many: 300 clients, a version after every 50
function manyDoc (seed) {
  const R = rng(seed + 5150); const ri = n => Math.floor(R() * n)
  const all = newDoc(5000); const versions = []
  for (let c = 0; c < 300; c++) {
    const d = newDoc(100 + 3 * c)
    d.getText('t').insert(0, 'p' + c + ALPH[ri(ALPH.length)]); if (c % 3 === 0) d.getText('t').delete(0, 1)
    Y.applyUpdate(all, Y.encodeStateAsUpdate(d))
    if (c % 50 === 49 && c < 299) versions.push(liveVersion(all))
  }
  all.getText('t').delete(2, 3)
  versions.push(liveVersion(all))
  all.getText('t').insert(0, 'end')
  return docRow('many', Y.encodeStateAsUpdate(all), versions)
}

// ---- pending: a lossy update stream; the versions a gc: false server took while it arrived
function pendingDoc (seed) {
  const R = rng(seed * 40503 + 7); const ri = n => Math.floor(R() * n)
  const d = newDoc(77 + ri(1000)); const log = []
  d.on('update', u => log.push(u))
  const t = d.getText('text')
  for (let k = 0; k < 24; k++) { if (t.length > 3 && R() < 0.3) t.delete(ri(t.length - 2), 2); else t.insert(ri(t.length + 1), ALPH[ri(ALPH.length)] + k) }
  const kept = log.slice(); kept.splice(14 + ri(4), 1)   // one update lost: what follows it stays pending
  const obs = new Y.Doc({ gc: false }); const versions = []
  kept.forEach((u, j) => { Y.applyUpdate(obs, u); if (j % 3 === 2) versions.push(liveVersion(obs)) })
  return docRow('pending', Y.mergeUpdates(kept), versions)
}

// ---- crafted: good versions, one ahead of the state, one taken from a different document
function craftedDoc (seed, foreign) {
  const R = rng(seed * 69069 + 3); const ri = n => Math.floor(R() * n)
  const d = newDoc(300 + ri(100)); const t = d.getText('text'); const versions = []; const notes = []
  for (let k = 0; k < 5; k++) {
    t.insert(ri(t.length + 1), 'w' + k + ALPH[ri(ALPH.length)]); if (k % 2) t.delete(0, 1)
    versions.push(liveVersion(d)); notes.push('good')
  }
  const state = Y.encodeStateAsUpdate(d)
  t.insert(0, 'later')
  versions.splice(2, 0, liveVersion(d)); notes.splice(2, 0, 'ahead of the state')
  versions.splice(4, 0, foreign); notes.splice(4, 0, 'from a different document')
  return docRow('crafted', state, versions, notes)
}

// ---- large: about 300 KB of long runs by two clients, versions between them
function largeDoc () {
  const a = newDoc(41); const b = newDoc(42); const versions = []
  for (let k = 0; k < 30; k++) {
    const d = k % 3 === 2 ? b : a
    d.getText('big').insert(k % 2 ? 0 : d.getText('big').length, String.fromCharCode(97 + k % 26).repeat(10000 + k))
    if (k % 5 === 4) { d.getText('big').delete(100 * k, 50); Y.applyUpdate(a, Y.encodeStateAsUpdate(b, Y.encodeStateVector(a))); Y.applyUpdate(b, Y.encodeStateAsUpdate(a, Y.encodeStateVector(b))); versions.push(liveVersion(a)) }
  }
  a.getText('big').insert(5, 'tail')
  return docRow('large', Y.encodeStateAsUpdate(a), versions)
}

if (require.main === module) {
  const out = process.argv[2]
  const seed = parseInt(process.argv[3] || '1', 10)
  const other = newDoc(9001); other.getText('text').insert(0, 'another document'); other.getText('text').delete(2, 3)
  const foreign = liveVersion(other)
  const docs = [textDoc(seed, 48)]
  for (let i = 0; i < 6; i++) docs.push(clientsDoc(seed + i, 3 + i % 3, 10))
  docs.push(manyDoc(seed))
  for (let i = 0; i < 3; i++) docs.push(pendingDoc(seed + i))
  for (let i = 0; i < 4; i++) docs.push(craftedDoc(seed + i, foreign))
  docs.push(docRow('empty', Uint8Array.from([0, 0]), [Uint8Array.from([0, 0])]))
  docs.push(largeDoc())
  const plain = u => { const d = new Y.Doc(); Y.applyUpdate(d, Buffer.from(u, 'hex')); return hex(Y.encodeStateAsUpdate(d)) }
  const fam = {}
  let answered = 0; let differ = 0
  for (const d of docs) {
    const f = fam[d.family] = fam[d.family] || { docs: 0, versions: 0, throws: 0, differ_from_snapshot: 0 }
    const p = plain(d.state)
    f.docs++
    for (const v of d.versions) {
      f.versions++
      if (v.restored === 'throws') f.throws++
      else { answered++; if (v.restored !== p) { f.differ_from_snapshot++; differ++ } }
    }
  }
  console.log(JSON.stringify(fam))
  if (differ * 10 < answered * 9) throw new Error('too few versions restore to bytes different from the plain snapshot: ' + differ + ' of ' + answered)
  fs.writeFileSync(out, zlib.gzipSync(Buffer.from(JSON.stringify({ yjs: '13.5.16', seed, docs })), { level: 9 }))
  const bytes = fs.statSync(out).size
  console.log(JSON.stringify({ docs: docs.length, versions: answered + docs.reduce((n, d) => n + d.versions.filter(v => v.restored === 'throws').length, 0), bytes }))
  if (bytes > 400 * 1024) throw new Error('the fixture is larger than 400 KB: ' + bytes)
}
